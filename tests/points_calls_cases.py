"""Inputs of tests/test_points_calls_gpu.py and tests/golden/make_points_calls_parent.py: every call that takes a CSR list of test
points (offsets, meta2, t2), the objectives that share their scatter and k_wgrad launch with them, at the smallest shapes that reach
every branch of the host helpers those calls share (medgp_capi.hip: check_points, upload_point_call, launch_pjvp_solve,
for_solved_chunks, download_mean_var*, launch_wgrad; call_plan.h: scatter_entry_blocks; capi.py: _point_args, _per_point, _split).

  A = tests/objective_calls_cases.py's family A: LMC-SM (7, 2, 2, 2), N = (40, 130, 70), the second patient uploaded interleaved: three
      size classes of one entry each, a non-identity order.  Test points per patient (70, 0, 5).
  R = its family R: N = (40, 130, 200): the ragged class of two entries (4 and 3 blocks) and a class of one.  Points (0, 5, 70): the two
      entries of the ragged class both have points, so the calls that cut their launch chunks between ENTRIES (posterior_vjp,
      posterior_joint) can be cut between them.
  S = SM (8, 2, 1, 1), N = (40, 100, 70), meta2_list = None (the library sees meta2 == NULL): a class of two entries (2 blocks each)
      and a class of one.  Points (0, 70, 5).
  70 points are two tiles of 64 with a partial last one (three of k_trend's 32, more of k_components'); 0 points is an entry
  without tiles.  "none" repeats four calls of family A with no point at all (M == 0).

Every (family, call) runs at the default MEDGP_POSTERIOR_BUDGET_GB and under a small one (budget_of), set before the context is
created: 1e-6 GB (below one tile's work rows: one launch per tile) for the calls whose chunks are runs of tiles, and for the two whose
chunks are whole entries (posterior_joint, posterior_vjp: they refuse an entry that does not fit alone) a value between the need of
the largest entry and the need of the two-entry class, so the cut falls between its entries.  chunk_label names the profile label
whose launch count shows the cut; CUT says whether a cut is possible (family A has no class of two entries).
"""
import os

import numpy as np

import medgp_amd
from medgp_amd import synth
import objective_calls_cases as OC

SM_FAMILY, SM_NS = (8, 2, 1, 1), (40, 100, 70)
FAMILIES = ("A", "R", "S")
POINTS = {"A": (70, 0, 5), "R": (0, 5, 70), "S": (0, 70, 5)}
PLAN = {"A": OC.PLAN["A"], "R": OC.PLAN["R"], "S": [(2, 2), (1, 1)]}
NS = {"A": OC.FAMILIES["A"][1], "R": OC.FAMILIES["R"][1], "S": SM_NS}
CLASSES_WITH_POINTS = {"A": 2, "R": 1, "S": 1}      # the classes whose entries have test points: the launches of a default-budget call
BUDGETS = ("default", "small")
TILE_BUDGET_GB = "1e-6"
KIB = 1.0 / 1024 / 1024
# bytes at once per entry, by inference_tables.h / pvjp_tables.h (ld = 64 x blocks of the class, nt tiles of 64 points, m points):
#   posterior_joint  nt ld 64 8 + (64 nt)^2 8 + m^2 4 (cov)      posterior_vjp  nt 2 ld 64 8
#   R (ld 256; 70 | 5 points): joint 412816 | 163940, vjp 524288 | 262144     S (ld 128; 70 | 5): joint 281744 | 98404, vjp 262144 | 131072
ENTRY_BUDGET_GB = {("A", "posterior_joint"): repr(600 * KIB), ("A", "posterior_vjp"): repr(600 * KIB),
                   ("R", "posterior_joint"): repr(500 * KIB), ("R", "posterior_vjp"): repr(600 * KIB),
                   ("S", "posterior_joint"): repr(300 * KIB), ("S", "posterior_vjp"): repr(300 * KIB)}
NCOT = NVEC = 2
PB = OC.PB
FAILED = 0      # the entry the mean / basis objectives make fail (LMC-SM families; S: the basis objective alone)
NONE_CALLS = ("posterior/parts", "posterior_vjp/nlpd", "mean_posterior/marginal", "warp_posterior/y2")


def data(fam):
    """(family, [(meta, t, y) per patient], theta [P, H], [basis [n, PB] per patient])"""
    if fam != "S":
        return OC.data(fam)
    pts = [synth.patient(11, p, 1, n) for p, n in enumerate(SM_NS)]
    th = np.stack([synth.theta(11, p, *SM_FAMILY) for p in range(len(SM_NS))])
    Hs = [np.stack([np.ones(t.shape[0]), t.astype(np.float64) / 200.0, (t > 100.0).astype(np.float64)], axis=1) for _, t, _ in pts]
    return SM_FAMILY, pts, th, Hs


def basis_rows(m, t, lmc):
    return np.stack([np.ones(t.shape[0]), t.astype(np.float64) / 200.0, ((m == 0) if lmc else (t > 100.0)).astype(np.float64)], axis=1)


def points(fam, none=False):
    """dict(m2 (None for S), t2, y2, h2, prefix, cm, cv, wt, eps, vecs) of the family's test points: one array per patient"""
    kf, pts, _, _ = data(fam)
    D, ns = kf[2], [p[1].shape[0] for p in pts]
    cnt = (0, 0, 0) if none else POINTS[fam]
    g = np.random.default_rng(29)
    m2 = [g.integers(0, D, size=m).astype(np.int32) for m in cnt]
    t2 = [g.uniform(0.0, 200.0, size=m).astype(np.float32) for m in cnt]
    out = dict(m2=m2 if kf[0] == 7 else None, t2=t2)
    out["y2"] = [g.normal(size=m) for m in cnt]
    out["h2"] = [basis_rows(m, t, kf[0] == 7) for m, t in zip(m2, t2)]
    # point j from the first prefix[j] observations in upload order: not sorted, so the call's sort and its scatter back are exercised
    out["prefix"] = [g.integers(0, n + 1, size=m).astype(np.int32) for m, n in zip(cnt, ns)]
    out["cm"] = [g.normal(size=(m, NCOT)) for m in cnt]
    out["cv"] = [g.normal(size=(m, NCOT)) for m in cnt]
    out["wt"] = [g.uniform(0.5, 2.0, size=m) for m in cnt]
    out["eps"] = [g.normal(size=(m, 3)) for m in cnt]
    out["vecs"] = g.normal(size=(len(cnt), NVEC, synth.num_hyp(*kf)))
    return out


def make_ctx(fam):
    """a fresh context with the family's patients and bases resident and every launch counted"""
    kf, pts, _, Hs = data(fam)
    ctx = medgp_amd.Context(*kf)
    ctx.reserve(len(pts), max(p[1].shape[0] for p in pts), len(pts))
    for s, (m, t, y) in enumerate(pts):
        ctx.set_patient(s, m if kf[0] == 7 else None, t, y)
    ctx.set_basis(np.arange(len(pts)), Hs)
    ctx.profile_enable(True)
    return ctx


def failing(fam):
    """what makes entry FAILED fail: (mean: the patient re-uploaded with every observation on covariate 0 and lam = 0 on covariate 1 --
    improper, as tests/fixed_effects_cases.py's lmc_D24; None for S, where D = 1), (basis: column 2 a copy of column 0 and both flat -- a
    failed pivot, as its "singular" case)"""
    kf, pts, _, Hs = data(fam)
    Hb = [h.copy() for h in Hs]
    Hb[FAILED][:, 2] = Hb[FAILED][:, 0]
    blam = np.tile(np.array([0.0, 1.0, 2.0]), (len(pts), 1))
    blam[FAILED, [0, 2]] = 0.0
    if kf[0] != 7:
        return None, (Hb, blam)
    m, t, y = pts[FAILED]
    mlam = np.tile(np.array([0.7, 1.3]), (len(pts), 1))
    mlam[FAILED, 1] = 0.0
    return ((np.zeros_like(m), t, y), mlam), (Hb, blam)


def calls(fam, none=False):
    """[(call name, f(ctx) -> result)]; each is made on a context of its own"""
    kf, pts, th, _ = data(fam)
    P, D = len(pts), kf[2]
    sl = np.arange(P)
    x = points(fam, none)
    m2, t2, vecs = x["m2"], x["t2"], x["vecs"]
    g = np.random.default_rng(31)
    mb0, mlam = 0.1 * g.normal(size=D), g.uniform(0.5, 2.0, size=D)
    bb0, blam = 0.1 * g.normal(size=PB), np.array([0.0, 1.0, 2.0])
    psi = np.stack([np.stack([g.uniform(-0.5, 0.5, D), g.uniform(-1.0, 1.0, D), g.uniform(-0.7, 0.7, D)], axis=1) for _ in range(P)])
    kind = np.array([medgp_amd.capi.WARP_SAS, medgp_amd.capi.WARP_NONE], np.int32) if D == 2 else None   # (S: its one covariate SAS)
    zq3 = [-1.0, 0.0, 1.5]
    out = [
        ("posterior/parts", lambda c: c.posterior(sl, th, m2, t2)),
        ("posterior/plain", lambda c: c.posterior(sl, th, m2, t2, parts=False)),
        ("posterior_joint/cov", lambda c: c.posterior_joint(sl, th, m2, t2)),
        ("posterior_joint/samples", lambda c: c.posterior_joint(sl, th, m2, t2, eps_list=x["eps"], cov=False)),
        ("forecast", lambda c: c.forecast(sl, th, m2, t2, prefix_list=x["prefix"], y2_list=x["y2"])),
        ("trend", lambda c: c.trend(sl, th, m2, t2)),
        ("components", lambda c: c.components(sl, th, m2, t2)),
        ("posterior_jvp/posterior", lambda c: c.posterior_jvp(sl, th, m2, t2, vecs)),
        ("posterior_jvp/bare", lambda c: c.posterior_jvp(sl, th, m2, t2, vecs, want_posterior=False)),
        ("posterior_vjp/custom", lambda c: c.posterior_vjp(sl, th, m2, t2, cot_mean=x["cm"], cot_var=x["cv"])),
        ("posterior_vjp/nlpd", lambda c: c.posterior_vjp(sl, th, m2, t2, loss="nlpd", y2_list=x["y2"])),
        ("posterior_vjp/nlpd_wt", lambda c: c.posterior_vjp(sl, th, m2, t2, loss="nlpd", y2_list=x["y2"], wt_list=x["wt"])),
        ("posterior_vjp/fp64", lambda c: c.posterior_vjp(sl, th, m2, t2, loss="nlpd", y2_list=x["y2"], fp64_posterior=True)),
        ("mean_posterior/marginal", lambda c: c.mean_posterior(sl, th, m2, t2, b0=mb0, lam=mlam)),
        ("mean_posterior/fixed", lambda c: c.mean_posterior(sl, th, m2, t2, b0=mb0, fixed=True)),
        ("basis_posterior/marginal", lambda c: c.basis_posterior(sl, th, m2, t2, x["h2"], b0=bb0, lam=blam)),
        ("basis_posterior/fixed", lambda c: c.basis_posterior(sl, th, m2, t2, x["h2"], b0=bb0, fixed=True)),
        ("warp_posterior/y2", lambda c: c.warp_posterior(sl, th, psi, m2, t2, y2_list=x["y2"], kind=kind, zq=zq3)),
        ("warp_posterior/bare", lambda c: c.warp_posterior(sl, th, psi, m2, t2, kind=kind, zq=[])),
    ]
    if none:
        return [c for c in out if c[0] in NONE_CALLS]
    fm, (Hb, fblam) = failing(fam)

    def mean_grad(c, fg):
        if fm is None:
            return c.mean_nlml_grad(sl, th, b0=mb0, lam=mlam, flag_grad=bool(fg))
        c.set_patient(FAILED, *fm[0])
        return c.mean_nlml_grad(sl, th, b0=mb0, lam=fm[1], flag_grad=bool(fg))

    def basis_grad(c, fg):
        c.set_basis(sl, Hb)
        return c.basis_nlml_grad(sl, th, b0=bb0, lam=fblam, flag_grad=bool(fg))

    for fg in (0, 1):
        out.append((f"warp_nlml_grad/{fg}", lambda c, fg=fg: c.warp_nlml_grad(sl, th, psi, kind=kind, flag_grad=bool(fg))))
        out.append((f"mean_nlml_grad/{fg}", lambda c, fg=fg: mean_grad(c, fg)))
        out.append((f"basis_nlml_grad/{fg}", lambda c, fg=fg: basis_grad(c, fg)))
    out.append(("nlml_grad", lambda c: c.nlml_grad(sl, th, True)))
    return out


CALL_NAMES = ["posterior/parts", "posterior/plain", "posterior_joint/cov", "posterior_joint/samples", "forecast", "trend", "components",
              "posterior_jvp/posterior", "posterior_jvp/bare", "posterior_vjp/custom", "posterior_vjp/nlpd", "posterior_vjp/nlpd_wt",
              "posterior_vjp/fp64", "mean_posterior/marginal", "mean_posterior/fixed", "basis_posterior/marginal", "basis_posterior/fixed",
              "warp_posterior/y2", "warp_posterior/bare", "warp_nlml_grad/0", "mean_nlml_grad/0", "basis_nlml_grad/0", "warp_nlml_grad/1",
              "mean_nlml_grad/1", "basis_nlml_grad/1", "nlml_grad"]
# (family, budget, call) of every recorded run: the objectives take no points, so no budget reaches them
RUNS = [(f, b, n) for f in FAMILIES for b in BUDGETS for n in CALL_NAMES if b == "default" or "nlml_grad" not in n] + \
       [("none", "default", n) for n in NONE_CALLS]


def chunk_label(name):
    """the profile label whose launches count the launch chunks of a call (posterior_vjp: k_pvjp_cot runs once per chunk and cotangent
    set, also on a chunk whose entries have no tile, where k_pjvp_solve is not launched)"""
    head = name.split("/")[0]
    return {"posterior": "k_posterior", "posterior_joint": "k_posterior", "components": "k_posterior", "forecast": "k_forecast",
            "trend": "k_trend", "posterior_vjp": "k_pvjp_cot"}.get(head, "k_pjvp_solve")


def cut_possible(fam, name):
    """whether the small budget can cut more launch chunks than the default one: not where chunks are whole entries and no class has two"""
    return not (fam == "A" and name.split("/")[0] in ("posterior_joint", "posterior_vjp"))


def budget_of(fam, budget, name):
    """the value of MEDGP_POSTERIOR_BUDGET_GB of a run (None: unset)"""
    if budget == "default":
        return None
    return ENTRY_BUDGET_GB.get((fam, name.split("/")[0]), TILE_BUDGET_GB)


def flat(x):
    """every array of a (nested) result, in a fixed order; None and plain numbers among them (a missing output stays visible)"""
    if isinstance(x, np.ndarray):
        return [x]
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (list, tuple)):
        return [a for y in x for a in flat(y)]
    return [np.zeros(0, np.uint8)] if x is None else [np.atleast_1d(np.asarray(x))]


def statuses(name, res):
    """the per-patient status array of a call's result"""
    if isinstance(res, dict):
        return res["status"]
    head = name.split("/")[0]
    return res[2] if head in ("mean_posterior", "basis_posterior", "nlml_grad") else res[1]


def run(fam, budget, name):
    """one call on a fresh context created under the run's budget: (arrays of the result, launch count per profile label, the call's size
    classes as (entries, 64-blocks of the largest), the result)"""
    none = fam == "none"
    f = dict(calls("A" if none else fam, none))[name]
    gb = budget_of(fam, budget, name)
    old = os.environ.pop("MEDGP_POSTERIOR_BUDGET_GB", None)
    if gb is not None:
        os.environ["MEDGP_POSTERIOR_BUDGET_GB"] = gb
    try:
        ctx = make_ctx("A" if none else fam)     # (the budget is read when the context is created)
    finally:
        os.environ.pop("MEDGP_POSTERIOR_BUDGET_GB", None)
        if old is not None:
            os.environ["MEDGP_POSTERIOR_BUDGET_GB"] = old
    try:
        ctx.profile_reset()
        res = f(ctx)
        prof = ctx.profile_read(all_entries=True)
        plan = [c[:2] for c in ctx.last_plan()]
    finally:
        ctx.close()
    return flat(res), {k: int(v[1]) for k, v in prof.items()}, plan, res
