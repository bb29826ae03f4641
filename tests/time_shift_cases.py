"""The inputs, references and the fp64 table restatement of the time-shift tests: every inference call at |t| up to 2^14 h, the limit
include/medgp_hip.h documents.  No device code is imported: tests/test_time_shift.py (CPU) vouches for what is here, and
tests/test_time_shift_gpu.py holds the device to it.

The covariance depends on time differences only, but the kernels form cos(w (t_i - t*)) as cs_i cc + sn_i sc from tables of cos / sin
(w t) at the times themselves.  So the same patient moved along the time axis has the same posterior and another rounding: the
references are computed once on the unshifted inputs (every existing restatement forms tau from differences, exact on the grid), the
device runs on the inputs moved by OFFSETS.

    families   T1h / T12h / T72h: nlml_truth.time_cases() (LMC-SM, Q = 3, D = 3, R = 2, n = 60 and 120); sm (SM, Q = 3, one component at
               each of the three periods); se; q17 (LMC-SM, Q = 17 at the 1 h period: the difference path of the point kernels)
    inputs     everything on the 2^-6 h grid within [-3, 203] h of the origin, so every shift is exact in float32 (asserted)
    tables_restate()   an fp64 program that forms K, K* (and K*') the device's way, from tables at the SHIFTED times; downstream as the
               references.  It shows the room a correct device has under the fp32 bar and measures what a legitimate fp64 program
               loses with |t| in the fp64 outputs (tests/golden/time_shift_spread.json, written by tests/golden/make_time_shift_spread.py)
"""
import functools
import json
import os

import numpy as np

from medgp_amd import functionals as FN
import components_ref as CR
import forecast_ref as FR
import functional_joint_ref as FJ
import functional_ref as FNR
import loo_grad_truth as LG
import loo_ref as LR
import nlml_truth as T
import posterior_joint_ref as PJ
import posterior_ref as PR
import trend_ref as TR

OFFSETS = [-2.0 ** 14, 0.0, 2.0 ** 10, 2.0 ** 14]
GRID = 64                   # times are multiples of 2^-6 h
M_POINTS = 70               # two tiles of 64, three of 32, four of 64 / Q for Q = 17
N_FUNCTIONALS = 70
N_SAMPLES = 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "time_shift_spread.json")
SPREAD_KEYS = ("forecast_lpd", "loo_lpd", "loo_obj", "loo_grad")
# The recorded errors are compared above these floors.  Below them an error is not the loss of the tables but the rounding of one fp64
# program on a matrix of cond(K) ~ 1e2 (the references of the lpd are fp64 themselves: forecast_ref.LPD_FLOOR; the gradient of a
# well-conditioned patient at the origin sits at 1e-13 .. 5e-12 in every legitimate fp64 program, loo_grad_truth.programs_of), which
# another BLAS or thread count moves by more than a factor of 2.  No bound of the GPU test is set by a value under its floor:
# F x floor is below the quantity's existing bound (50 x 1e-12 < 1e-10 for the LOO lpd, 128 x 1e-11 ~ the gradient cap 2^-30) except
# for the forecast lpd, whose bound reads the committed file, not this floor.
SPREAD_FLOOR = {"forecast_lpd": 1e-12, "loo_lpd": 1e-12, "loo_obj": 1e-13, "loo_grad": 1e-11}
ROOM = 0.25                 # fp32 ulps the table program may use of the 2-ulp bar

FAMILIES = ["T1h", "T12h", "T72h", "sm", "se", "q17"]


def _grid_patient(g, n):
    t = np.sort(g.integers(0, 200 * GRID, size=n) / float(GRID)).astype(np.float32)
    return None, t, g.standard_normal(n).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(id, kidx, Q, D, R, pts = [(meta, t, y)], th = [theta], period) as nlml_truth's cases; treat as read-only"""
    for c in T.time_cases():
        if c["id"] == f"time_{name}":
            return dict(c, id=name)
    g = T._philox(20261201, FAMILIES.index(name))
    if name == "sm":       # theta = [log sigma | log weight | log mu | log v]: one component per period of nlml_truth.TIME_PERIODS
        Q = 3
        th = np.concatenate([[np.log(g.uniform(0.15, 0.4))], np.log(g.uniform(0.1, 0.5, size=Q)), np.log(1.0 / np.array(T.TIME_PERIODS)),
                             np.log(1.0 / (2 * T.REF_PI * np.exp(g.uniform(np.log(6.0), np.log(72.0), size=Q))))])
        return dict(id=name, sweep="time", kidx=8, Q=Q, D=1, R=0, pts=[_grid_patient(g, 120)], th=[th], period=1.0)
    if name == "se":       # theta = [log sigma | log l | log sf]
        th = np.log([g.uniform(0.15, 0.4), g.uniform(6.0, 24.0), g.uniform(0.7, 1.3)])
        return dict(id=name, sweep="time", kidx=0, Q=1, D=1, R=0, pts=[_grid_patient(g, 120)], th=[th], period=None)
    if name == "q17":
        D, Q, R, n = 3, 17, 2, 100
        m = np.sort(g.integers(0, D, size=n)).astype(np.int32)
        t = (g.integers(0, 200 * GRID, size=n) / float(GRID)).astype(np.float32)
        for d in range(D):
            idx = np.where(m == d)[0]
            t[idx] = np.sort(t[idx])
        pts = [(m, t, g.standard_normal(n).astype(np.float32))]
        th = [T._lmc_theta(T._philox(20261202, 0), Q, D, R, period=1.0, scale=(6.0, 72.0), noise=(0.15, 0.4))]
        return dict(id=name, sweep="time", kidx=7, Q=Q, D=D, R=R, pts=pts, th=th, period=1.0)
    raise KeyError(name)


def fam(c):
    return c["kidx"], c["Q"], c["D"], c["R"]


def patients(name):
    return range(len(case(name)["pts"]))


def has_loo_grad(c):
    return c["Q"] <= 16        # medgp_loo_grad supports Q <= 16


def _snap(t):
    return (np.round(np.asarray(t, np.float64) * GRID) / GRID).astype(np.float32)


@functools.lru_cache(maxsize=None)
def call_inputs(name, p):
    """the per-patient inputs of every call, unshifted, all on the grid; read-only.  dict(m2, t2, prefix, y2, packed, eps)"""
    c = case(name)
    D = c["D"]
    m, t, y = c["pts"][p]
    n = t.shape[0]
    g = T._philox(20261203, 16 * FAMILIES.index(name) + p)
    M = M_POINTS
    t2 = (g.integers(-3 * GRID, 203 * GRID + 1, size=M) / float(GRID)).astype(np.float32)
    m2 = g.integers(0, D, size=M).astype(np.int32)
    prefix = g.integers(0, n + 1, size=M).astype(np.int32)
    prefix[0], prefix[1] = 0, n
    y2 = g.standard_normal(M).astype(np.float32)
    fs = []
    for j in range(N_FUNCTIONALS):          # the callers' kinds of functional_cases.mix, node times snapped to the grid
        mm = int(g.integers(0, D))
        tt = float(g.integers(-3 * GRID, 203 * GRID + 1)) / GRID
        t0 = float(g.integers(-3 * GRID, 179 * GRID + 1)) / GRID
        kind = j % 5
        if kind == 0:
            f = FN.point(mm, tt)
        elif kind == 1:
            f = FN.window_mean(mm, t0, t0 + 24.0, 25)
        elif kind == 2:
            f = FN.change(mm, t0, t0 + 6.0)
        elif kind == 3:
            f = FN.change(mm, t0, t0 + 0.25)
        else:
            f = FN.contrast((mm, tt), ((mm + 1) % D, tt)) if D > 1 else FN.contrast((0, t0), (0, t0 + 12.0))
        fs.append((f[0], _snap(f[1]), f[2]))
    packed = FN.pack(fs)
    assert np.all(packed[2] >= -3.0) and np.all(packed[2] <= 203.0)
    eps = g.standard_normal((M, N_SAMPLES))
    return dict(m2=m2, t2=t2, prefix=prefix, y2=y2, packed=packed, eps=eps)


def shift_times(t, off):
    """float32 times moved by off, asserted exact (as nlml_truth.shifted)"""
    t = np.asarray(t, np.float32)
    t2 = (t.astype(np.float64) + off).astype(np.float32)
    assert np.all(t2.astype(np.float64) - off == t.astype(np.float64)), "offset not exact in float32"
    return t2


def shifted(name, p, off):
    """((meta, t, y), inputs) of patient p with the observations (nlml_truth.shifted), the test times and the functionals' node times
    moved by off"""
    c = case(name)
    pt = T.shifted(dict(c, pts=[c["pts"][p]]), off)["pts"][0]
    q = dict(call_inputs(name, p))
    q["t2"] = shift_times(q["t2"], off)
    toff, fm, ft, fa = q["packed"]
    q["packed"] = (toff, fm, shift_times(ft, off), fa)
    return pt, q


# ---- the references: the existing restatements, once per patient on the unshifted inputs ---------------------------------------------

def restatements(c, p, pt, q, X=np.longdouble):
    """every output of every call from the existing restatements on (pt, q); X: the precision of the ones that take a dtype"""
    f = fam(c)
    kidx = f[0]
    m, t, y = pt
    th = c["th"][p]
    multi = kidx == 7
    m2 = q["m2"] if multi else None
    toff, fm, ft, fa = q["packed"]
    fm = fm if multi else None
    out = {}
    out["posterior"] = PR.restate(*f, m, t, y, th, m2, q["t2"])
    out["joint"] = PJ.restate_joint(*f, m, t, y, th, m2, q["t2"])
    out["samples"] = PJ.draw(out["joint"], q["eps"])
    out["loo"] = LR.refit(*f, m, t, y, th)
    out["loo_cov"] = LR.refit(*f, m, t, y, th, *covariate_groups(c, pt))
    out["loo_grad"] = LG.loo_grad(*f, m, t, y, th, np.longdouble) if has_loo_grad(c) else None
    out["forecast"] = FR.refit(*f, m, t, y, th, m2, q["t2"], q["prefix"], q["y2"])
    out["trend"] = TR.restate(*f, m, t, y, th, m2, q["t2"], dtype=X)
    out["components"] = CR.restate(*f, m, t, y, th, m2, q["t2"], dtype=X)
    out["functional"] = FNR.restate(*f, m, t, y, th, toff, fm, ft, fa, dtype=X)
    out["functional_joint"] = FJ.restate(*f, m, t, y, th, toff, fm, ft, fa, dtype=X)
    return out


def covariate_groups(c, pt):
    """(group ids, number of groups) of leave-one-covariate-out (one all-inclusive group for SE / SM)"""
    n = pt[1].shape[0]
    return (np.asarray(pt[0], np.int64), c["D"]) if c["kidx"] == 7 else (np.zeros(n, np.int64), 1)


@functools.lru_cache(maxsize=None)
def reference(name, p):
    c = case(name)
    return restatements(c, p, c["pts"][p], call_inputs(name, p))


# ---- the table restatement -------------------------------------------------------------------------------------------------------------

class _Tables:
    """the Gram blocks the device's way, in fp64: cos(w d) = cs_a cs_b + sn_a sn_b from cos / sin (w t) at the times as given.
    side "train": k_prep's row tables; side "test": the tables of the test points / terms (with phase32: w t* rounded to float32, the
    mutant of the rejection test).  diff_test: the test side takes cos / sin of the difference instead (the generic component loop)."""

    def __init__(self, c, p, phase32=False, diff_test=False):
        self.sig2, self.B, self.w, self.c = TR.hypers(*fam(c), c["th"][p], np.float64)
        self.Q = c["Q"]
        self.phase32, self.diff_test = phase32, diff_test

    def tab(self, t, side):
        ph = self.w[:, None] * t[None, :]
        if side == "test" and self.phase32:
            ph = ph.astype(np.float32).astype(np.float64)
        return np.cos(ph), np.sin(ph)

    def gram(self, ma, ta, sa, mb, tb, sb, slope=False, q=None, diff=False):
        """K[i, j] = sum_q B_q[ma_i, mb_j] cos(w_q d) exp(-c_q d^2), d = ta_i - tb_j (slope: and d / d tb_j of it); q: one component"""
        d = ta[:, None] - tb[None, :]
        ca, na = self.tab(ta, sa)
        cb, nb = self.tab(tb, sb)
        K = np.zeros(d.shape)
        Kd = np.zeros(d.shape) if slope else None
        for k in (range(self.Q) if q is None else [q]):
            Bs = self.B[k][ma[:, None], mb[None, :]]
            e = np.exp(-self.c[k] * d * d)
            if diff:
                cd, sd = np.cos(self.w[k] * d), np.sin(self.w[k] * d)
            else:
                cd = ca[k][:, None] * cb[k][None, :] + na[k][:, None] * nb[k][None, :]
                sd = na[k][:, None] * cb[k][None, :] - ca[k][:, None] * nb[k][None, :]
            K += Bs * (cd * e)
            if slope:
                Kd += Bs * ((self.w[k] * sd + (2.0 * self.c[k] * d) * cd) * e)
        return (K, Kd) if slope else K


def _loo_from_gram(K, y, ids, G, pi=T.REF_PI):
    """loo_ref.refit on a given Gram matrix"""
    n = K.shape[0]
    mean, var, lpd = np.full(n, np.nan), np.full(n, np.nan), np.zeros(G)
    for gid in range(G):
        Bi = np.flatnonzero(ids == gid)
        if Bi.size == 0:
            continue
        rest = np.flatnonzero(ids != gid)
        if rest.size:
            Lr = np.linalg.cholesky(K[np.ix_(rest, rest)])
            A = np.linalg.solve(Lr, K[np.ix_(rest, Bi)])
            mu = A.T @ np.linalg.solve(Lr, y[rest])
            Cb = K[np.ix_(Bi, Bi)] - A.T @ A
            Cb = 0.5 * (Cb + Cb.T)
        else:
            mu, Cb = np.zeros(Bi.size), K[np.ix_(Bi, Bi)]
        mean[Bi], var[Bi] = mu, np.diag(Cb)
        lpd[gid] = LR._gauss_logpdf(y[Bi] - mu, Cb, pi)
    return mean, var, lpd, float(lpd.sum())


def _loo_grad_tables(c, p, pt):
    """loo_grad_truth.loo_grad in float64 with nlml_truth's cosine tables (k_prep's) in K and in the gradient factors"""
    f = fam(c)
    kidx, Q, D, R = f
    m, t, y = pt
    th = c["th"][p]
    X = np.float64
    t32 = np.asarray(t, np.float32)
    yy = np.asarray(y, np.float32).astype(X)
    K = T.gram(*f, m, t32, th, X, 0, tables=True)
    Li = T._tri_inverse(T._chol_blocked64(K))
    P = T._gram_upper_product(Li)
    alpha = Li.T @ (Li @ yy)
    J = LG._from_inverse(*f, m, t32, th, P, alpha, X, False, None)[0]
    d = np.diagonal(P)
    s = (1 + alpha * alpha / d) / d
    v = P @ (alpha / d)
    W = (P * s[None, :]) @ P - alpha[:, None] * v[None, :] - v[:, None] * alpha[None, :]
    W = (W + W.T) / 2
    # the W -> g lines of nlml_truth.nlml_grad, factors from the tables
    h = T.transform(*f, th, X)
    tt = t32.astype(X)
    n = tt.shape[0]
    dt = tt[:, None] - tt[None, :]
    g = np.zeros(T.num_hyp(*f), X)
    wd = np.diagonal(W)
    if kidx == 7:
        mm = np.asarray(m, np.int64)
        E = np.zeros((n, D), X)
        E[np.arange(n), mm] = 1
        g[:D] = h["sig2"] * (wd @ E)
        o_mu, o_v, o_k = D + Q * D * R, D + Q * D * R + Q, D + Q * (D * R + 2)
        for k in range(Q):
            kk, km, kv = T._sm_factors(h, k, tt, dt, True)
            S = E.T @ ((W * kk) @ E)
            g[D + k * D * R:D + (k + 1) * D * R] = (((S + S.T) / 2) @ h["A"][k]).ravel()
            WB = W * h["B"][k][mm[:, None], mm[None, :]]
            g[o_mu + k] = np.sum(WB * km) / 2
            g[o_v + k] = np.sum(WB * kv) / 2
            g[o_k + k * D:o_k + (k + 1) * D] = h["kappa"][k] * np.diagonal(S) / 2
    elif kidx == 8:
        g[0] = h["sig2"][0] * np.sum(wd)
        for k in range(Q):
            for j, fct in enumerate(T._sm_factors(h, k, tt, dt, True)):
                g[1 + j * Q + k] = h["w"][k] * np.sum(W * fct) / 2
    else:
        return LG.loo_grad(*f, m, t, y, th, X)      # SE has no tables
    return J, g


def tables_restate(name, p, off, phase32=False):
    """Every output of every call for patient p moved by off, in fp64 with K, K* (and K*') from cos / sin tables at the shifted times
    (class _Tables); the same keys and layouts as restatements().  Downstream of the Gram blocks it follows the references.  For
    Q > 8 the point kernels (posterior, joint, forecast, trend) take cos / sin of the difference on the test side, as the device."""
    c = case(name)
    pt, q = shifted(name, p, off)
    kidx, Q, D, R = fam(c)
    multi = kidx == 7
    m, t, y = pt
    n, M = t.shape[0], q["t2"].shape[0]
    tb = _Tables(c, p, phase32)
    ta = np.asarray(t, np.float32).astype(np.float64)
    yy = np.asarray(y, np.float32).astype(np.float64)
    ma = np.asarray(m, np.int64) if multi else np.zeros(n, np.int64)
    t2 = q["t2"].astype(np.float64)
    m2 = q["m2"].astype(np.int64) if multi else np.zeros(M, np.int64)
    gen = Q > 8
    Kn = tb.gram(ma, ta, "train", ma, ta, "train")
    Kxx = Kn.copy()
    Kxx[np.diag_indices(n)] += tb.sig2[ma]
    Lc = np.linalg.cholesky(Kxx)
    z = np.linalg.solve(Lc, yy)
    alpha = np.linalg.solve(Lc.T, z)
    Ks, Kd = tb.gram(ma, ta, "train", m2, t2, "test", slope=True, diff=gen)
    kss = np.sum(tb.B[:, m2, m2], axis=0)
    sig2_2 = tb.sig2[m2]
    V = np.linalg.solve(Lc, Ks)
    out = {}
    # posterior_ref.restate
    mean = Ks.T @ alpha
    var = kss - np.sum(V * V, axis=0) + sig2_2
    Dp = D if multi else 1
    parts = np.zeros((M, Dp))
    for d in range(Dp):
        parts[:, d] = Ks[ma == d].T @ alpha[ma == d]
    out["posterior"] = (mean, var, parts)
    # posterior_joint_ref.restate_joint
    Kss = tb.gram(m2, t2, "test", m2, t2, "test", diff=gen)
    Kss[np.diag_indices(M)] += sig2_2
    C = Kss - V.T @ V
    C = 0.5 * (C + C.T)
    out["joint"] = (V.T @ z, np.diag(C).copy(), C, np.linalg.cholesky(C))
    out["samples"] = PJ.draw(out["joint"], q["eps"])
    # loo_ref.refit
    out["loo"] = _loo_from_gram(Kxx, yy, np.arange(n), n)
    ids, G = covariate_groups(c, pt)
    out["loo_cov"] = _loo_from_gram(Kxx, yy, ids, G)
    out["loo_grad"] = _loo_grad_tables(c, p, pt) if has_loo_grad(c) else None
    # forecast_ref.refit
    fm, fv = np.zeros(M), np.zeros(M)
    for pf in np.unique(q["prefix"]):
        sel = np.flatnonzero(q["prefix"] == pf)
        if pf == 0:
            fv[sel] = kss[sel] + sig2_2[sel]
            continue
        Lp = np.linalg.cholesky(Kxx[:pf, :pf])
        Vp = np.linalg.solve(Lp, Ks[:pf][:, sel])
        fm[sel] = Ks[:pf][:, sel].T @ np.linalg.solve(Lp.T, np.linalg.solve(Lp, yy[:pf]))
        fv[sel] = kss[sel] - np.sum(Vp * Vp, axis=0) + sig2_2[sel]
    out["forecast"] = (fm, fv, FR.log_density(q["y2"], fm, fv))
    # trend_ref.restate (K*' = d / dt* of K*)
    Vd = np.linalg.solve(Lc, Kd)
    prior = np.zeros(M)
    for k in range(Q):
        prior += tb.B[k][m2, m2] * (tb.w[k] * tb.w[k] + 2.0 * tb.c[k])
    out["trend"] = (V.T @ z, var, Vd.T @ z, prior - np.sum(Vd * Vd, axis=0), -np.sum(V * Vd, axis=0), prior)
    # components_ref.restate (tables for every Q)
    Vq = np.stack([np.linalg.solve(Lc, tb.gram(ma, ta, "train", m2, t2, "test", q=k)) for k in range(Q)], axis=1)      # [n, Q, M]
    cprior = np.stack([tb.B[k][m2, m2] for k in range(Q)], axis=1)
    ccov = -np.einsum("iqj,irj->jqr", Vq, Vq)
    ccov[:, np.arange(Q), np.arange(Q)] += cprior
    out["components"] = (np.einsum("iqj,i->jq", Vq, z), ccov[:, np.arange(Q), np.arange(Q)].copy(), ccov, cprior)
    # functional_ref.restate / functional_joint_ref.restate (tables for every Q; the priors from the differences, as the device)
    toff, fmeta, ft, fa = q["packed"]
    ft = ft.astype(np.float64)
    fmeta = fmeta.astype(np.int64) if multi else np.zeros(ft.shape[0], np.int64)
    F = toff.shape[0] - 1
    A = np.zeros((ft.shape[0], F))
    for f in range(F):
        A[int(toff[f]):int(toff[f + 1]), f] = fa[int(toff[f]):int(toff[f + 1])]
    Vg = np.linalg.solve(Lc, tb.gram(ma, ta, "train", fmeta, ft, "test") @ A)
    Qp = A.T @ (tb.gram(fmeta, ft, "test", fmeta, ft, "test", diff=True) @ A)
    Qp = (Qp + Qp.T) / 2
    fcov = Qp - Vg.T @ Vg
    fcov = (fcov + fcov.T) / 2
    out["functional"] = (Vg.T @ z, np.diag(Qp) - np.sum(Vg * Vg, axis=0), np.diag(Qp).copy())
    out["functional_joint"] = (Vg.T @ z, np.diag(fcov).copy(), fcov, Qp)
    return out


# ---- errors ----------------------------------------------------------------------------------------------------------------------------

def fp32_errors(c, pt, out, ref):
    """{output name: error in fp32 ulps of max(|ref|, 1e-3 S)} of every fp32 output of every call (the scales of the checkers)"""
    e = {}
    for k, nm in enumerate(("mean", "var", "parts")):
        e[f"posterior.{nm}"] = PR.ulp_error(out["posterior"][k], ref["posterior"][k])
    e["joint.cov"] = PR.ulp_error(out["joint"][2], ref["joint"][2])
    e["joint.samples"] = PR.ulp_error(out["samples"], ref["samples"])
    for key in ("loo", "loo_cov"):
        em, ev, _ = LR.errors(ref[key], pt[2], out[key])
        e[f"{key}.mean"], e[f"{key}.var"] = em, ev
    e["forecast.mean"] = PR.ulp_error(out["forecast"][0], ref["forecast"][0])
    e["forecast.var"] = PR.ulp_error(out["forecast"][1], ref["forecast"][1])
    for k, nm in enumerate(TR.NAMES):
        e[f"trend.{nm}"] = PR.ulp_error(out["trend"][k], np.asarray(ref["trend"][k], np.float64))
    for k, nm in enumerate(CR.NAMES):
        e[f"components.{nm}"] = PR.ulp_error(out["components"][k], np.asarray(ref["components"][k], np.float64))
    for k, nm in enumerate(FNR.NAMES):
        e[f"functional.{nm}"] = PR.ulp_error(out["functional"][k], np.asarray(ref["functional"][k], np.float64))
    e["functional_joint.fcov"] = PR.ulp_error(out["functional_joint"][2], np.asarray(ref["functional_joint"][2], np.float64))
    return e


def fp64_errors(c, pt, out, ref):
    """{SPREAD_KEYS: error} of the fp64 outputs in the scale of each quantity's existing bar: lpd relative to max(1, |ref|)
    (forecast_ref.lpd_error, loo_ref.errors), objective and gradient as nlml_truth.error_pair"""
    e = {"forecast_lpd": FR.lpd_error(out["forecast"][2], ref["forecast"][2]),
         "loo_lpd": max(LR.errors(ref[k], pt[2], out[k])[2] for k in ("loo", "loo_cov"))}
    if ref["loo_grad"] is not None:
        e["loo_obj"], e["loo_grad"] = T.error_pair(out["loo_grad"][0], out["loo_grad"][1], *ref["loo_grad"])
    return e


def off_key(off):
    return str(int(off))


def measure_spread():
    """{family: {offset: {SPREAD_KEYS: worst error of tables_restate over the family's patients}}}: what the golden file holds"""
    res = {}
    for name in FAMILIES:
        c = case(name)
        res[name] = {}
        for off in OFFSETS:
            worst = {}
            for p in patients(name):
                e = fp64_errors(c, c["pts"][p], tables_restate(name, p, off), reference(name, p))
                for k, x in e.items():
                    worst[k] = max(worst.get(k, 0.0), x)
            res[name][off_key(off)] = worst
    return res


@functools.lru_cache(maxsize=None)
def recorded_spread():
    with open(GOLDEN) as fh:
        return json.load(fh)["spread"]


@functools.lru_cache(maxsize=None)
def loo_grad_budget(name, p):
    """(objective budget, gradient budget) of the patient at offset 0, as loo_grad_truth.budget_of measures it: M x the worse of the two
    legitimate fp64 programs, capped"""
    c = case(name)
    m, t, y = c["pts"][p]
    tj, tg = reference(name, p)["loo_grad"]
    b = LG.loo_grad(*fam(c), m, t, y, c["th"][p], np.float64)
    cc = LG.loo_grad_linalg(*fam(c), m, t, y, c["th"][p])
    e = [T.error_pair(b[0], b[1], tj, tg), T.error_pair(cc[0], cc[1], tj, tg)]
    return (min(T.budget([x[0] for x in e], LG.M_OBJ), T.NLML_BUDGET_CAP), min(T.budget([x[1] for x in e], LG.M_GRAD), T.GRAD_BUDGET_CAP))


def fp64_bounds(name, p, off):
    """{SPREAD_KEYS: bound} of the device at an offset: max(the quantity's existing bound, F x the recorded error of the table program
    at that (family, offset)).  The device and the table program share the dominant error, the rounding of the tables; F (the factor the
    project already gives the quantity over a legitimate fp64 program) covers the summation order."""
    rec = recorded_spread()[name][off_key(off)]
    b = {"forecast_lpd": max(FR.lpd_bound(), FR.LPD_FACTOR * rec["forecast_lpd"]),
         "loo_lpd": max(LR.LPD_BOUND, FR.LPD_FACTOR * rec["loo_lpd"])}
    if has_loo_grad(case(name)):
        bj, bg = loo_grad_budget(name, p)
        b["loo_obj"] = max(bj, LG.M_OBJ * rec["loo_obj"])
        b["loo_grad"] = max(bg, LG.M_GRAD * rec["loo_grad"])
    return b
