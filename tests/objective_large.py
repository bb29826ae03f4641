"""The four gradient objectives -- medgp_loo_grad, medgp_lgo_grad, medgp_forecast_grad, medgp_fisher_vec -- above N = 512: the cases,
their committed long-double truths and their fp64 budgets, shared by tests/test_objective_large.py (CPU: the fixture and the budget
conditions) and tests/test_objective_large_gpu.py (the device held to the budgets).

The patients and hyper vectors are those of nlml_truth.large_cases(), taken by id (inputs come from seeds alone), plus one D = 64
patient drawn from the next seed index of that sweep.  The truths are those of loo_grad_truth, lgo_grad_truth and fisher_truth as they
stand; the forecast truth is forecast_grad_truth's definition with ONE factorisation shared by all history lengths
(forecast_grad_shared below: the leading p x p block of the column Cholesky factor of K IS the column Cholesky factor of K[0:p, 0:p],
operation for operation, and so is its triangular inverse; tests/test_objective_large.py holds the two to the same long-double bits).
The refit of every history length costs n factorisations, an hour per entry at n = 1024.

Budgets follow each objective's own module, unchanged: M_OBJ = 256, M_GRAD = 128, M_FISHER = 128; the budget of an entry is
M * max(E_b, E_c), floored at M * 2^-53, where (b) is the truth code in float64 and (c) the numpy.linalg program (the one-factor
program for the forecast), both measured against the truth on the CPU alone.  The caps -- M max(E_b, E_c) <= GRAD_BUDGET_CAP and
NLML_BUDGET_CAP, cond(K) <= COND_MAX -- are conditions on the INPUTS, asserted by the CPU test; no min(budget, cap) here.

The truths are too slow for a test (n = 1024: LOO 12 s, Fisher 22 s a direction, n = 2048 minutes each), so they are committed:
tests/golden/make_objective_truth_large.py writes tests/golden/objective_truth_large.npz, by hand; entry() raises on a missing key
or a changed input hash and never recomputes.
"""
import hashlib
import os

import numpy as np

import fisher_truth as FT
import forecast_grad_truth as FG
import lgo_grad_truth as GG
import loo_grad_truth as LG
import nlml_truth as T
from loo_grad_truth import COND_MAX, M_GRAD, M_OBJ   # noqa: F401
from fisher_truth import M_FISHER   # noqa: F401
from nlml_truth import GRAD_BUDGET_CAP, NLML_BUDGET_CAP, U64, budget, error_pair   # noqa: F401

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective_truth_large.npz")
OBJECTIVES = ["loo", "lgo", "fc", "fisher"]
HORIZONS = {"h0": 0.0, "h6": 6.0, "h48": 48.0}     # 48 h of a 200 h stay: bands of about a quarter of n
NVEC = FT.NVEC

# the new patient of leg wideD, seeded as the LMC cases of nlml_truth.large_cases() are, at the next case index
WIDE_ID, WIDE_CI, WIDE_FAM, WIDE_SPEC = "large_wideD", len(T._LARGE_LMC), (7, 2, 64, 2), [(200, "missing")]
CASE_ORDER = ["large_pass2", "large_q_Q8", "large_q_Q9", "large_q_Q16", WIDE_ID, "large_sm_Q4", "large_se", "large_config3"]

# Which hyper draw a (case id, patient, objective) uses where it is not the one nlml_truth.DRAWS gives the patient: the first of the
# eight draws k = 0 .. 7 of nlml_truth's rule (synth.theta(seed + 1000 k, ...)) on which every table of that objective meets the caps
# above, found on the CPU programs alone (the maker prints a miss; tests/test_objective_large.py re-checks the entries as they stand).
DRAWS = {
    ("large_q_Q8", 0, "fc"): 2,        # draws 0 and 1 (nlml_truth's): the 0 h gradient budget 1.66e-9 / 9.75e-10 against the cap of 9.31e-10
    ("large_q_Q8", 0, "lgo"): 2,       # draws 0 and 1: scheme cov 1.61e-9 / 1.32e-9
    ("large_q_Q9", 0, "fc"): 1,        # draw 0: the 6 h gradient budget 2.05e-9
    ("large_q_Q16", 0, "fc"): 2,       # draw 0: 0 h 9.41e-10; draw 1: 6 h 1.31e-9
    ("large_q_Q16", 0, "lgo"): 2,      # draw 0: cov 1.21e-9; draw 1: win 1.95e-9
    ("large_config3", 0, "loo"): 2,    # draw 0: 1.24e-9; draw 1: 9.82e-10
}

# (case id, patient, objective) pairs for which none of the eight draws meets the caps (at most two, none in leg pass2): DESIGN.md section 3
DROPPED = set()
# the optional entries of the n = 2048 leg that the maker did not finish within 30 minutes: DESIGN.md section 3
LONG_OPTIONAL = [("large_config3", 0, "lgo", "cov"), ("large_config3", 0, "fc", "h6")]
LONG_ABSENT = set()

# ---- the leave-group-out block limit (inference_tables.h) -----------------------------------------------------------------------------
DEFAULT_POSTERIOR_BUDGET = 2 << 30          # bytes: medgp_capi.hip, MEDGP_POSTERIOR_BUDGET_GB unset
CAP_BUDGET_GB = 15.0 / 1024.0               # 15 MiB: the budget under which the limit falls inside an n = 1024 patient (960 rows)


def loo_block_bytes(m):
    """bytes of the block of a group of m >= 2 members: inference_tables.h, loo_block_doubles (2 mpad^2 + 2 mpad doubles)"""
    mpad = (m + 63) // 64 * 64
    return 8 * (2 * mpad * mpad + 2 * mpad)


def group_limit(budget_bytes):
    """the largest group build_loo_tables admits: it refuses a group when loo_block_bytes(m) > budget"""
    m = 64
    while loo_block_bytes(m + 64) <= budget_bytes:
        m += 64
    return m


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _theta(cid, p, k):
    """draw k of patient p of a case, by nlml_truth.large_cases()'s seeds"""
    from medgp_amd import synth
    if cid == WIDE_ID:
        return synth.theta(4714 + 1000 * k, 100 * WIDE_CI + p, *WIDE_FAM)
    if cid in ("large_sm_Q4", "large_se"):
        kidx, Q = (8, 4) if cid == "large_sm_Q4" else (0, 1)
        return synth.theta(4715 + 1000 * k, kidx, kidx, Q, 1, 0)
    ci = [c[0] for c in T._LARGE_LMC].index(cid)
    _, Q, D, R, _ = T._LARGE_LMC[ci]
    return synth.theta(4714 + 1000 * k, 100 * ci + p, 7, Q, D, R)


def draw_of(cid, p, obj):
    return DRAWS.get((cid, p, obj), T._draw(cid, p))


def base_case(cid):
    """the case of nlml_truth.large_cases() with this id (or the wideD case), patients in upload order grouped by covariate"""
    if cid not in _CASES:
        if cid == WIDE_ID:
            from random_patients import random_patient
            g = T._philox(20261023, WIDE_CI)
            kidx, Q, D, R = WIDE_FAM
            pts = [random_patient(g, D, n, mode) for n, mode in WIDE_SPEC]
            _CASES[cid] = dict(id=cid, sweep="large", kidx=kidx, Q=Q, D=D, R=R, pts=pts, th=[_theta(cid, p, T._draw(cid, p)) for p in range(len(pts))])
        else:
            for c in T.large_cases():
                _CASES[c["id"]] = c
    return _CASES[cid]


def case(cid, obj):
    """the case as objective obj sees it: the objective's hyper draws; for the forecast every patient stably sorted by time (as
    forecast_grad_truth.case)"""
    key = (cid, obj)
    if key not in _CASES:
        c = base_case(cid)
        th = [c["th"][p] if draw_of(cid, p, obj) == T._draw(cid, p) else _theta(cid, p, draw_of(cid, p, obj)) for p in range(len(c["pts"]))]
        pts = c["pts"]
        if obj == "fc":
            pts = []
            for m, t, y in c["pts"]:
                o = np.argsort(t, kind="stable")
                pts.append((None if m is None else m[o], t[o], y[o]))
        _CASES[key] = dict(c, pts=pts, th=th)
    return _CASES[key]


fam = LG.fam


def n_of(cid, p):
    return base_case(cid)["pts"][p][1].shape[0]


# ---- the entries: (leg, case id, patient, objective, table) ------------------------------------------------------------------------------
# table: loo "-" | lgo: a scheme of group_table() | fc: a key of HORIZONS | fisher: "v<number of directions>"
LGO_SCHEMES = ["cov", "win"]


def _four(leg, cid, p, lgo=True, nvec=NVEC):
    out = [(leg, cid, p, "loo", "-"), (leg, cid, p, "fisher", f"v{nvec}")]
    out += [(leg, cid, p, "fc", h) for h in HORIZONS]
    if lgo:
        out += [(leg, cid, p, "lgo", s) for s in LGO_SCHEMES]
    return out


def all_entries():
    """every entry the issue's case list demands, optional and dropped ones included"""
    E = []
    for p in range(4):
        E += _four("pass2", "large_pass2", p)
    E += [("pass2", "large_pass2", 1, "lgo", "one"),          # (b) one group at n = 576: the nlml
          ("pass2", "large_pass2", 3, "lgo", "max"),          # (c) the largest group the default budget admits at n = 1024
          ("pass2", "large_pass2", 3, "lgo", "cap960")]       #     and the largest under CAP_BUDGET_GB, the rest singletons
    for cid in ("large_q_Q8", "large_q_Q9", "large_q_Q16"):
        E += _four("qsplit", cid, 0)
    E += [("qsplit", "large_q_Q9", 0, "lgo", "two320")]       # (a) two interleaved groups of 320 at n = 640
    E += _four("wideD", WIDE_ID, 0)
    for cid in ("large_sm_Q4", "large_se"):
        E += _four("single", cid, 0, lgo=False)
    E += [("long", "large_config3", 0, "loo", "-"), ("long", "large_config3", 0, "fisher", "v1")]
    E += [("long",) + k for k in LONG_OPTIONAL]
    return E


def entries(leg=None, obj=None):
    """the entries the fixture must hold: all_entries() without the dropped pairs and the absent optional ones"""
    return [e for e in all_entries()
            if e[1:4] not in DROPPED and e[1:] not in LONG_ABSENT and (leg is None or e[0] == leg) and (obj is None or e[3] == obj)]


def key_of(e):
    return "%s:%d:%s:%s" % tuple(e[1:])


def group_table(cid, p, scheme):
    """(group ids in upload order, ngroups) of a scheme, from seeds alone"""
    c = case(cid, "lgo")
    n = n_of(cid, p)
    if scheme in ("cov", "win"):
        return GG.groups_of(c, p, scheme)
    if scheme == "one":
        return np.zeros(n, np.int32), 1
    g = T._philox(20261401, 1000 * CASE_ORDER.index(cid) + p)
    if scheme == "two320":
        assert n == 640
        ids = np.zeros(n, np.int32)
        ids[g.permutation(n)[:320]] = 1
        return ids, 2
    lim = {"max": group_limit(DEFAULT_POSTERIOR_BUDGET), "cap960": group_limit(int(CAP_BUDGET_GB * 1073741824.0))}[scheme]
    big = min(lim, n)                             # the largest single group admitted, the rest singletons
    ids = np.zeros(n, np.int32)
    ids[g.permutation(n)[big:]] = 1 + np.arange(n - big)
    return ids, 1 + n - big


def one_past(cid, p, scheme):
    """the table of group_table with one more row in its large group (n > limit); None when the patient has no row to add"""
    ids, ng = group_table(cid, p, scheme)
    if ng == 1:
        return None
    ids = ids.copy()
    ids[np.flatnonzero(ids == ng - 1)] = 0
    return ids, ng - 1


def directions(cid, p, nvec):
    """nvec standard-normal directions, from seeds alone; direction j does not depend on nvec (as fisher_truth.directions)"""
    H = T.num_hyp(*fam(base_case(cid)))
    return np.array([T._philox(20261402, 1000 * CASE_ORDER.index(cid) + 10 * p + j).standard_normal(H) for j in range(nvec)])


def table_of(e):
    """what the call of entry e takes beside the patient and theta: None (loo) | (group, ngroups) | prefix | directions [nvec, H]"""
    _, cid, p, obj, tab = e
    if obj == "loo":
        return None
    if obj == "lgo":
        return group_table(cid, p, tab)
    if obj == "fc":
        return FG.prefix_of(case(cid, "fc"), p, HORIZONS[tab])
    return directions(cid, p, int(tab[1:]))


def input_sha256(e):
    """SHA-256 of the exact input bytes of an entry: nlml_truth.input_sha256's bytes of the patient as the objective sees it, then the
    objective's name and its table (group ids and count as int32, prefix as int32, directions as float64)"""
    _, cid, p, obj, tab = e
    c = case(cid, obj)
    h = hashlib.sha256()
    h.update(bytes.fromhex(T.input_sha256(c, p)))
    h.update(obj.encode())
    tb = table_of(e)
    if obj == "lgo":
        h.update(np.ascontiguousarray(tb[0], np.int32).tobytes())
        h.update(np.array([tb[1]], np.int32).tobytes())
    elif obj == "fc":
        h.update(np.ascontiguousarray(tb, np.int32).tobytes())
    elif obj == "fisher":
        h.update(np.ascontiguousarray(tb, np.float64).tobytes())
    return h.hexdigest()


# ---- the forecast truth on one shared factorisation ------------------------------------------------------------------------------------

def forecast_grad_shared(kidx, Q, D, R, meta, t, y, theta, prefix=None, dtype=np.longdouble, jitter_rounds=0):
    """forecast_grad_truth.forecast_grad with the factor of every history length read off ONE column Cholesky of K: column j of
    nlml_truth._chol_columns takes rows j.. of K and of the columns before it, row by row, so its first p rows are the factor of
    K[0:p, 0:p] bit for bit, and row i of nlml_truth._tri_inverse takes the rows above it alone.  (J, grad) in precision dtype."""
    X = dtype
    t32 = np.asarray(t, np.float32)
    n = t32.shape[0]
    form = "naive" if n <= LG.NAIVE_MAX_N else "blocks"
    pf = FG._check_prefix(prefix, n)
    yy = np.asarray(y, np.float32).astype(X)
    K = T.gram(kidx, Q, D, R, meta, t32, theta, X, jitter_rounds)
    log2pi = np.log(2 * T.transform(kidx, Q, D, R, theta, X)["pi"])
    scored = np.flatnonzero(pf >= 0)
    lpd = np.zeros(n, X)
    Um, Bm = np.zeros((n, scored.shape[0]), X), np.zeros((n, scored.shape[0]), X)
    g, e = np.zeros(scored.shape[0], X), np.zeros(scored.shape[0], X)
    col = {int(i): c for c, i in enumerate(scored)}
    Lall = T._tri_inverse(T._chol_columns(K))
    for p in np.unique(pf[scored]):
        p = int(p)
        if p > 0:
            Li = Lall[:p, :p]
            beta = Li.T @ (Li @ yy[:p])
        for i in np.flatnonzero(pf == p):
            i = int(i)
            c = col[i]
            Um[i, c] = 1
            if p > 0:
                a = Li.T @ (Li @ K[:p, i])
                Um[:p, c] = -a
                Bm[:p, c] = beta
                mean, var = a @ yy[:p], K[i, i] - K[:p, i] @ a
            else:
                mean, var = X(0), K[i, i]
            r = yy[i] - mean
            lpd[i] = -(log2pi + np.log(var)) / 2 - r * r / var / 2
            g[c] = (1 - r * r / var) / var
            e[c] = r / var
    J = -np.sum(lpd)
    W = FG._w_fc(Um, Bm, g, e)
    return J, LG.grad_from_w(kidx, Q, D, R, meta, t32, theta, W, X, form)


# ---- truth and the two fp64 programs of an entry ---------------------------------------------------------------------------------------

def run_program(e, which):
    """entry e by program "truth" (long double), "b" (the truth code in float64) or "c" (numpy.linalg; the forecast: one factor).
    (obj, grad[H]) -- the Fisher call: (None, fvec[nvec, H])"""
    _, cid, p, obj, tab = e
    c = case(cid, obj)
    f = fam(c)
    m, t, y = c["pts"][p]
    th = c["th"][p]
    tb = table_of(e)
    X = np.longdouble if which == "truth" else np.float64
    if obj == "loo":
        return LG.loo_grad_linalg(*f, m, t, y, th) if which == "c" else LG.loo_grad(*f, m, t, y, th, X)
    if obj == "lgo":
        return GG.lgo_grad_linalg(*f, m, t, y, th, *tb) if which == "c" else GG.lgo_grad(*f, m, t, y, th, *tb, X)
    if obj == "fc":
        return FG.one_factor(*f, m, t, y, th, tb) if which == "c" else forecast_grad_shared(*f, m, t, y, th, tb, X)
    return None, (FT.fisher_vec_linalg(*f, m, t, th, tb) if which == "c" else FT.fisher_vec(*f, m, t, th, tb, X))


def errors_of(e, got, truth):
    """(E_obj or None, E_grad) of one program's output against the truth, on each objective's own scale"""
    if e[3] == "fisher":
        return None, FT.errors(got[1], truth[1])
    return error_pair(got[0], got[1], truth[0], truth[1])


def cond_of(cid, p, obj):
    c = case(cid, obj)
    m, t, _ = c["pts"][p]
    return LG.cond(*fam(c), m, t, c["th"][p])


# ---- the committed fixture -------------------------------------------------------------------------------------------------------------
_FIXTURE = None


def fixture():
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(FIXTURE) as z:
            _FIXTURE = {k: z[k] for k in z.files}
        _FIXTURE["_index"] = {str(k): i for i, k in enumerate(_FIXTURE["keys"])}
    return _FIXTURE


def entry(e):
    """dict(truth = (obj, grad) in long double (the Fisher call: (None, [nvec, H])), en = [E_b, E_c] or None, eg = [E_b, E_c], cond)
    of a committed entry.  Raises (never skips, never recomputes) when the entry is missing or was made from other input bytes."""
    z = fixture()
    key = key_of(e)
    if key not in z["_index"]:
        raise RuntimeError(f"{FIXTURE} holds no truth for {key}: run tests/golden/make_objective_truth_large.py")
    i = z["_index"][key]
    sha = input_sha256(e)
    if str(z["sha256"][i]) != sha:
        raise RuntimeError(f"{FIXTURE}: {key} was computed from other inputs (stored {z['sha256'][i]}, now {sha}): "
                           "run tests/golden/make_objective_truth_large.py")
    X = np.longdouble
    tg = z[f"grad_hi_{i}"].astype(X) + z[f"grad_lo_{i}"].astype(X)
    fisher = e[3] == "fisher"
    tj = None if fisher else X(z["obj_hi"][i]) + X(z["obj_lo"][i])
    return dict(truth=(tj, tg), en=None if fisher else [float(x) for x in z["en"][i]], eg=[float(x) for x in z["eg"][i]],
                cond=float(z["cond"][i]))


def budgets(e):
    """(truth obj or None, truth grad, objective budget or None, gradient budget) of an entry: M * max(E_b, E_c), floored at M * U64"""
    r = entry(e)
    if e[3] == "fisher":
        return None, r["truth"][1], None, budget(r["eg"], M_FISHER)
    return r["truth"][0], r["truth"][1], budget(r["en"], M_OBJ), budget(r["eg"], M_GRAD)
