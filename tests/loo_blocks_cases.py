"""Inputs of tests/test_loo_blocks_bits_gpu.py and tests/golden/make_loo_blocks_parent.py: the leave-group-out calls on family R of
tests/objective_calls_cases.py (N = 40, 130, 200, the second patient interleaved) with groups on both sides of every block count the
group kernels distinguish (k_loo_gram, k_postfactor, k_loo_solve; k_lgo_inv, k_lgo_s, k_lgo_t: 64-row blocks of a group's index list).

The N = 40 and N = 130 patients keep the groups of objective_calls_cases (a row never held out, a singleton, an empty id, groups of
2 .. 64 and, N = 130, the group of 70: two blocks, the second one padded).  The N = 200 patient is to hold a row never held out, an
empty id, a singleton, a group of 2, one of exactly 64, one of 65 and one of 135 (three blocks: the smallest count at which the sum
over c <= j < k of the block-column inverse has more than one term and the tile pair (2, 1) exists).  Those are 268 rows, a patient
has 200, and a row has one group: so the patient gets TWO layouts, and every call with groups is made once with each:
  "small"  1 never held out, id 1 empty, a singleton, a pair, 64, 65, and the remaining 67 rows as one more group
  "large"  1 never held out, 135, 64
Members are spread over the patient's rows by a fixed permutation (no group is a contiguous run).

Calls: loo_batch with mean, var and lpd together (Context.loo), with var alone and with mean and lpd alone (the C entry point with NULL
outputs: the early returns of k_loo_solve's two job kinds), classic leave-one-out (no groups), lgo_grad with flag_grad 0 and 1.
"""
import ctypes as C

import numpy as np

from medgp_amd import capi
import objective_calls_cases as OC

FAM = "R"
LAYOUTS = {"small": (("never", 1), (0, 1), (2, 2), (3, 64), (4, 65), (5, 67)),      # id 1 stays empty
           "large": (("never", 1), (0, 135), (1, 64))}


def groups(layout):
    """one int32 array of group ids per patient of family R"""
    ns = OC.FAMILIES[FAM][1]
    out = OC._groups(ns[:2])
    order = np.random.default_rng(23).permutation(ns[2])
    gid = np.empty(ns[2], dtype=np.int32)
    at = 0
    for g, cnt in LAYOUTS[layout]:
        gid[order[at:at + cnt]] = -1 if g == "never" else g
        at += cnt
    assert at == ns[2]
    return out + [gid]


def loo_raw(ctx, slots, th, grp, want):
    """medgp_loo_batch with only the outputs named in `want` (of mean, var, lpd, total) non-NULL: {name: array}, plus status and
    group_status"""
    slots, th, ns, gs, ng = ctx._loo_args(slots, th, grp)
    nb, NO, NG = slots.shape[0], int(sum(ns)), int(sum(ns) if gs is None else ng.sum())
    g = None if gs is None else np.ascontiguousarray(np.concatenate(gs), dtype=np.int32)
    out = {k: np.empty(n, dtype=ty) for k, n, ty in (("mean", NO, np.float32), ("var", NO, np.float32), ("lpd", NG, np.float64),
                                                      ("total", nb, np.float64)) if k in want}
    st, gst = np.empty(nb, dtype=np.int32), np.empty(NG, dtype=np.int32)
    p = lambda k, ty: capi._ptr(out.get(k), ty)
    ctx._chk(ctx._lib.medgp_loo_batch(ctx._h, nb, capi._ptr(slots, C.c_int32), capi._ptr(th, C.c_double), capi._ptr(g, C.c_int32),
                                      capi._ptr(ng, C.c_int32), p("mean", C.c_float), p("var", C.c_float), p("lpd", C.c_double),
                                      p("total", C.c_double), capi._ptr(st, C.c_int32), capi._ptr(gst, C.c_int32)))
    out.update(status=st, group_status=gst)
    return out


def calls():
    """[(call name, f(ctx) -> result)]"""
    _, pts, th, _ = OC.data(FAM)
    slots = np.arange(len(pts))
    out = [("loo/none", lambda c: c.loo(slots, th, None))]
    for lay in LAYOUTS:
        grp = groups(lay)
        out.append((f"loo/{lay}/all", lambda c, grp=grp: c.loo(slots, th, grp)))
        out.append((f"loo/{lay}/var", lambda c, grp=grp: loo_raw(c, slots, th, grp, ("var",))))
        out.append((f"loo/{lay}/mean_lpd", lambda c, grp=grp: loo_raw(c, slots, th, grp, ("mean", "lpd"))))
        for fg in (0, 1):
            out.append((f"lgo_grad/{lay}/{fg}", lambda c, grp=grp, fg=fg: c.lgo_grad(slots, th, grp, fg)))
    return out


def statuses(name, res):
    """the per-patient status array of a call's result"""
    if isinstance(res, dict):
        return res["status"]
    return res[2] if name.startswith("lgo_grad") else res[1]


def run_fresh():
    """every call on a context of its own: {call: (arrays, counts, result, plan)}"""
    out = {}
    for cname, f in calls():
        ctx = OC.make_ctx(FAM)
        try:
            out[cname] = OC.run_one(ctx, f)
        finally:
            ctx.close()
    return out
