"""medgp_posterior_vjp_batch without a GPU: the closed-form long-double truth (posterior_vjp_truth.py) against its definition (the JVP
truth on unit directions) and against Richardson differences of the long-double built-in losses, the scale identity, CRPS against
numerical integration of its definition, the conditions under which the fp64 error budget may be used to judge the device
(test_posterior_vjp_gpu.py), medgp_amd/predictive.py on analytic inputs, the ABI surface, and the host geometry's own test program."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from medgp_amd import capi, predictive
import loo_grad_truth as LG
import nlml_truth as T
import posterior_jvp_truth as PJ
import posterior_vjp_truth as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medgp_amd", "csrc")
X = np.longdouble

# patients whose full gradient by definition (H unit directions in long double) takes seconds: H <= 102, n <= 130
SMALL = [("lmc_sizes", 0), ("lmc_sizes", 2), ("lmc_sizes", 4), ("lmc_Q9", 0), ("sm_Q4", 0), ("se", 0)]


def _inputs(cid, p, count=None):
    c = PV.case(cid)
    m, t, y = c["pts"][p]
    m2, t2 = PV.points(c, p, count)
    return c, PV.fam(c), m, t, y, c["th"][p], m2, t2


def test_the_cases_meet_every_tile_edge_and_both_kinds_of_missing_covariate():
    counts = {PV.points(PV.case(cid), p)[1].shape[0] for cid, p in PV.patients()}
    assert {0, 1, 63, 64, 65, 130} <= counts
    c = PV.case("lmc_D24_missing")
    m2, _ = PV.points(c, 0)
    obs, tst = set(np.asarray(c["pts"][0][0]).tolist()), set(m2.tolist())
    assert obs - tst, "a covariate with observations and no test point"
    assert tst - obs, "a covariate with test points and no observation"
    assert m2.shape[0] > 64 and list(m2) != sorted(m2)          # two point tiles, unsorted as given
    assert any(c["kidx"] == 7 and c["Q"] in (9, 16) for c in map(PV.case, PV.CASE_IDS))


@pytest.mark.parametrize("cid,p", SMALL, ids=[f"{c}-{p}" for c, p in SMALL])
def test_closed_form_is_the_definition(cid, p):
    """every hyper: the closed form against sum_j cm_j dmean_j(e_h) + cv_j dvar_j(e_h) of the JVP truth, both in long double; a
    missing or mis-signed term errs at order 1 on the scale of the terms, rounding at 1e-19 times a condition number"""
    c, fam, m, t, y, th, m2, t2 = _inputs(cid, p)
    cm, cv = PV.cotangents(c, p)
    g, mag = PV.truth_of(c, p)
    d = PV.by_definition(*fam, m, t, y, th, m2, t2, cm, cv)
    assert PV.groups_nonzero(c, g) and PV.groups_nonzero(c, d)
    assert PV.error_of(d, g, mag) <= 1e-13
    assert np.all(mag >= np.abs(g) * (1 - 1e-12))               # the scale bounds the value: it is a sum of absolute values


@pytest.mark.parametrize("cid", ["lmc_D24_missing", "lmc_D24_n512"])
def test_closed_form_is_the_definition_on_a_subset_of_hypers_at_D24(cid):
    c, fam, m, t, y, th, m2, t2 = _inputs(cid, 0)
    cm, cv = PV.cotangents(c, 0)
    g, mag = PV.truth_of(c, 0)
    from medgp_amd.sensitivity import groups
    rng = T._philox(20261603, 0)
    hs = np.concatenate([rng.choice(np.arange(s.start, s.stop), size=min(3 if cid.endswith("n512") else 6, s.stop - s.start), replace=False)
                         for _, s in groups(*fam)])
    if cid == "lmc_D24_missing":     # the noise line and a kappa line of the covariate that has test points and no observation
        b = min(set(m2.tolist()) - set(np.asarray(m).tolist()))
        hs = np.concatenate([hs, [b, c["D"] + c["Q"] * (c["D"] * c["R"] + 2) + b]])
        assert g[0, b] != 0
    d = PV.by_definition(*fam, m, t, y, th, m2, t2, cm, cv, hs)
    scale = PJ.scale_of(mag[0])
    for k in range(PV.NCOT):
        assert float(np.max(np.abs(d[k] - g[k, hs]) / PJ.scale_of(mag[k])[hs])) <= 1e-13
    assert scale.min() > 0


def _loss_ld(kind, cid, p, th, y2, wt):
    c, fam, m, t, y, _, m2, t2 = _inputs(cid, p)
    mean, var = PJ.posterior(*fam, m, t, y, th, m2, t2, X)
    return predictive.BUILTIN[kind](mean, var, np.asarray(y2).astype(X), np.asarray(wt).astype(X))[0]


@pytest.mark.parametrize("kind", ["nlpd", "sqerr", "crps"])
@pytest.mark.parametrize("cid,p", [("lmc_sizes", 2), ("sm_Q4", 0), ("se", 0)], ids=["lmc", "sm", "se"])
def test_truth_is_the_gradient_of_the_builtin_loss(kind, cid, p):
    """Central differences of the long-double loss along v at steps h = 2^-8 and h / 2, Richardson-combined.  theta is stored in
    fp64, so each quotient is compared with grad . u for the direction u its two points really span.  The plain difference's error
    falls about 4 x from h to h / 2."""
    c, fam, m, t, y, th, m2, t2 = _inputs(cid, p)
    y2, wt = PV.targets(c, p)
    mean, var = PV.posterior_of(c, p)
    _, cm, cv = predictive.BUILTIN[kind](mean, var, y2.astype(X), wt.astype(X))
    g = PV.truth_for(c, p, cm, cv)[0][0]
    v = PJ.directions(c, p)[0]
    v = v / np.linalg.norm(v)

    def quot(step):
        a, b = th + step * v, th - step * v
        u = (a.astype(X) - b.astype(X)) / X(2 * step)
        return (_loss_ld(kind, cid, p, a, y2, wt) - _loss_ld(kind, cid, p, b, y2, wt)) / X(2 * step), u

    d1, u1 = quot(2.0 ** -8)
    d2, u2 = quot(2.0 ** -9)
    e1, e2 = abs(d1 - g @ u1), abs(d2 - g @ u2)
    rich = (4 * d2 - d1) / 3
    ref = (4 * (g @ u2) - g @ u1) / 3
    scale = float(np.sum(np.abs(g * u1)))
    assert scale > 0
    # a missing or mis-signed term errs at order 1 on this scale; the truncation of R is h^4 = 2e-10 times the ratio of the loss's
    # fifth to its first derivative along v (the periodic components make it some tens), the fp64 erf of the CRPS adds 1e-16 / h
    assert abs(rich - ref) <= 1e-7 * scale, (float(rich), float(ref))
    if e1 > 1e-9 * scale:
        assert 3.0 <= float(e1 / e2) <= 5.0, float(e1 / e2)


@pytest.mark.parametrize("cid,p", [("lmc_sizes", 4), ("lmc_D24_missing", 0), ("sm_Q4", 0), ("se", 0)])
def test_scale_direction_of_the_custom_gradient(cid, p):
    """Scaling the kernel and the noise together leaves the mean and scales the variance: along s (the direction d log scale) the
    gradient is  sum_j cv_j 2 var_j  (dmean . s = 0, dvar . s = 2 var)"""
    c, fam, m, t, y, th, m2, t2 = _inputs(cid, p)
    kidx, Q, D, R = fam
    H = T.num_hyp(*fam)
    cm, cv = PV.cotangents(c, p)
    g, mag = PV.truth_of(c, p)
    _, var = PV.posterior_of(c, p)
    if kidx == 7:        # sigma, A and sqrt(kappa) scale together: d log sigma = 1, dA = A, d log kappa = 2
        s = np.zeros(H, X)
        s[:D] = 1
        s[D:D + Q * D * R] = np.asarray(th[D:D + Q * D * R]).astype(X)
        s[D + Q * (D * R + 2):] = 2
    elif kidx == 8:      # d log sigma = 1, d log w = 2
        s = np.zeros(H, X)
        s[0], s[1:1 + Q] = 1, 2
    else:                # d log sigma = 1, d log sf = 1
        s = np.array([1, 0, 1], X)
    for k in range(PV.NCOT):
        want = np.sum(cv[:, k].astype(X) * 2 * var)
        assert abs(g[k] @ s - want) <= 1e-13 * float(np.abs(mag[k] * np.abs(s)).sum())


def test_crps_and_its_cotangents_against_numerical_integration():
    """CRPS(F, y) = int (F(x) - 1[x >= y])^2 dx for F = N(mean, var), by the trapezoidal rule on fine grids; the cotangents against
    central differences of that integral"""
    def crps_int(mean, var, y):
        s = math.sqrt(var)
        erf = np.vectorize(math.erf)

        def part(a, b, upper):      # the integrand is smooth on either side of y: the grids end exactly there
            x = np.linspace(a, b, 200001)
            F = 0.5 * (1 + erf((x - mean) / (s * math.sqrt(2))))
            f = (1 - F) ** 2 if upper else F ** 2
            return float(np.sum((f[1:] + f[:-1]) / 2 * np.diff(x)))
        return part(min(mean - 12 * s, y - 1), y, False) + part(y, max(mean + 12 * s, y + 1), True)

    for mean, var, y in [(0.0, 1.0, 0.3), (1.5, 0.25, -0.2), (-2.0, 4.0, 1.0), (0.1, 0.01, 0.12), (3.0, 2.0, 3.0)]:
        val, cm, cv = predictive.crps(np.array([mean]), np.array([var]), np.array([y]))
        assert abs(val - crps_int(mean, var, y)) <= 2e-5 * max(1.0, abs(val))
        h = 1e-3
        dm = (crps_int(mean + h, var, y) - crps_int(mean - h, var, y)) / (2 * h)
        dv = (crps_int(mean, var * (1 + h), y) - crps_int(mean, var * (1 - h), y)) / (2 * h * var)
        assert abs(cm[0] - dm) <= 2e-4 and abs(cv[0] - dv) <= 2e-4 * max(1.0, abs(dv))


@pytest.mark.parametrize("name", ["nlpd", "sqerr", "crps", "pinball", "interval"])
def test_loss_cotangents_are_their_derivatives(name):
    f = {"pinball": predictive.pinball(0.9), "interval": predictive.interval_score(0.1)}.get(name) or predictive.BUILTIN[name]
    g = T._philox(20261604, 0)
    mean, var, y, wt = g.standard_normal(7), g.uniform(0.5, 2.0, 7), g.standard_normal(7), g.uniform(0.5, 1.5, 7)
    val, cm, cv = f(mean, var, y, wt)
    h = 1e-6
    for j in range(7):
        e = np.zeros(7)
        e[j] = h
        assert abs((f(mean + e, var, y, wt)[0] - f(mean - e, var, y, wt)[0]) / (2 * h) - cm[j]) <= 1e-7
        assert abs((f(mean, var + e, y, wt)[0] - f(mean, var - e, y, wt)[0]) / (2 * h) - cv[j]) <= 1e-7
    assert abs(f(mean, var, y)[0] - f(mean, var, y, np.ones(7))[0]) == 0


def test_budget_factor_M_and_caps():
    """The two float64 programs over all cases and one jitter round: their spread decides M_PVJP by the rule of the issue (keep
    M_GRAD = 128 if the spread is <= M / 4, else the smallest power of two >= 4 x the spread); every budget stays under the cap and
    every truth has a non-zero magnitude in the noise, coefficient, mu and v groups."""
    worst, who = 1.0, None
    runs = [(cid, p, 0) for cid, p in PV.patients()] + [("lmc_sizes", 5, 1), ("sm_Q4", 0, 1)]
    for cid, p, jr in runs:
        c = PV.case(cid)
        r = PV.programs_of(c, p, jr)
        (g, mag), bud = PV.budget_of(c, p, jr)
        assert bud <= PV.GRAD_BUDGET_CAP and all(np.isfinite(r["eg"]))
        if PV.points(c, p)[1].shape[0]:
            assert PV.groups_nonzero(c, g), (cid, p)
            sp = PV.spread(r["eg"])
            if sp > worst:
                worst, who = sp, (cid, p, jr)
        else:
            assert not g.any() and not mag.any()

    def rule(spread):
        M = 1
        while M < 4 * spread:
            M *= 2
        return M

    print(f"spread between the programs: {worst:.1f} at {who} -> M_PVJP {max(LG.M_GRAD, rule(worst))}")
    assert worst <= PV.M_PVJP / 4
    assert PV.M_PVJP == max(LG.M_GRAD, rule(worst))
    assert abs(worst - PV.MEASURED_SPREAD) <= 0.05 * PV.MEASURED_SPREAD + 0.1


# ---- the ABI surface and the host geometry -------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_posterior_vjp(built_lib):
    src = open(os.path.join(ROOT, "include", "medgp_hip.h")).read()
    assert re.search(r"int\s+medgp_posterior_vjp_batch\s*\(", src)
    assert "tests/posterior_vjp_truth.py" in src
    for k, name in enumerate(["CUSTOM", "NLPD", "SQERR", "CRPS"]):
        assert re.search(rf"#define\s+MEDGP_PLOSS_{name}\s+{k}\b", src)
    assert hasattr(C.CDLL(built_lib), "medgp_posterior_vjp_batch")
    assert "medgp_posterior_vjp_batch" in capi.SYMBOLS
    lib = capi.load()
    assert lib.medgp_abi_version() >= 19
    assert lib.medgp_profile_num_kernels() == 23          # the frozen table
    assert lib.medgp_profile_num_kernels_all() == 29      # ... and the one behind it
    names = [lib.medgp_profile_kernel_name(k).decode() for k in range(lib.medgp_profile_num_kernels_ext())]
    assert names[43:46] == ["k_pjvp_solve", "k_pjvp_u", "k_pjvp_dir"]
    assert names[46:50] == ["k_pvjp_cot", "k_pvjp_wgrad", "k_pvjp_cross", "k_pvjp_finish"]          # appended behind id 45
    blob = open(built_lib, "rb").read()
    assert all(n.encode() in blob for n in names[46:50])
    assert hasattr(capi.Context, "posterior_vjp") and capi.Context.PLOSS == {"custom": 0, "nlpd": 1, "sqerr": 2, "crps": 3}


def test_null_arguments_are_argument_errors(built_lib):
    """without a context every call is an argument error (-1) before any device work"""
    lib = capi.load()
    slots = np.zeros(1, np.int32)
    th = np.zeros(8)
    off = np.zeros(2, np.int64)
    ip, dp, lp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    a = (slots.ctypes.data_as(ip), th.ctypes.data_as(dp), off.ctypes.data_as(lp))
    d = th.ctypes.data_as(dp)
    assert lib.medgp_posterior_vjp_batch(None, 1, *a, None, None, 0, None, None, 1, d, d, None, None, None, d, None) == -1
    assert lib.medgp_posterior_vjp_batch(None, 1, *a, None, None, 1, d, None, 1, None, None, None, None, d, d, None) == -1
    assert lib.medgp_posterior_vjp_batch(None, 1, None, None, None, None, None, 7, None, None, 0, None, None, None, None, None, None, None) == -1


def test_host_geometry_under_sanitizers():
    """pvjp_tables.h (the by-covariate order, the tile table, the per-entry records, the chunks cut between entries, buffer sizes, the
    capacity rules) against restatements: a stand-alone program built with the host compiler under -fsanitize=address,undefined
    and started as an ordinary child process"""
    subprocess.check_call(["make", "-s", "-C", CSRC, "pvjp_tables_test"])
    out = subprocess.run([os.path.join(CSRC, "pvjp_tables_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pvjp_tables ok" in out.stdout
