"""ctypes binding of libmedgp_hip.so (C ABI: include/medgp_hip.h).

Mirrors the reference's call shape: a Context plays the role of the (kernel, likelihood,
inference, prior) object set of main_one_train.cpp:103-152, `set_patient` of
c_objective_one's constructor, `nlml_grad` of c_objective_one::compute_objective.
Fails loudly when the HIP library is missing -- there is no CPU path.
"""
import ctypes as C
import weakref
import os
from types import SimpleNamespace

import numpy as np

KERNEL_SE, KERNEL_LMC_SM, KERNEL_SM = 0, 7, 8
PRIOR_NONE, PRIOR_CLAMP, PRIOR_NORMAL, PRIOR_LAPLACE = -1, 0, 1, 2
FLAG_GRAD, FLAG_KEEP_FACTOR = 1, 2   # flag_grad bits (include/medgp_hip.h)
MEAN_MARGINAL, MEAN_FIXED = 0, 1     # mode of the baseline calls (include/medgp_hip.h)
WARP_NONE, WARP_SAS = 0, 1           # kind of a covariate in the warp calls (include/medgp_hip.h)

_HERE = os.path.dirname(os.path.abspath(__file__))

# every symbol include/medgp_hip.h declares (tests check the .so exports all of them)
SYMBOLS = [
    "medgp_abi_version", "medgp_device_count", "medgp_create", "medgp_destroy", "medgp_last_error",
    "medgp_num_hyp", "medgp_set_pi", "medgp_set_stream", "medgp_reserve", "medgp_reserve_plan", "medgp_alloc_stats", "medgp_set_patient",
    "medgp_set_patients", "medgp_set_prior", "medgp_set_priors", "medgp_host_alloc", "medgp_host_free", "medgp_nlml_grad_async",
    "medgp_wait", "medgp_nlml_grad", "medgp_screen", "medgp_nlml_grad_device", "medgp_get_factor",
    "medgp_factor", "medgp_factor_batch", "medgp_pin_route", "medgp_last_plan", "medgp_fit_predict", "medgp_fit_predict_batch", "medgp_posterior_batch", "medgp_posterior_joint_batch", "medgp_loo_batch", "medgp_loo_grad", "medgp_lgo_grad", "medgp_fisher_vec", "medgp_hess_vec", "medgp_posterior_jvp_batch", "medgp_posterior_vjp_batch", "medgp_posterior_vjp_moments", "medgp_mean_nlml_grad", "medgp_mean_posterior_batch", "medgp_set_basis", "medgp_basis_nlml_grad", "medgp_basis_posterior_batch", "medgp_warp_nlml_grad", "medgp_warp_posterior_batch", "medgp_set_noise_scale", "medgp_hetero_nlml_grad", "medgp_hetero_posterior_batch", "medgp_robust_nlml_grad", "medgp_forecast_batch", "medgp_forecast_grad", "medgp_trend_batch", "medgp_components_batch", "medgp_functional_batch", "medgp_functional_joint_batch", "medgp_synchronize", "medgp_profile_enable", "medgp_profile_num_kernels", "medgp_profile_num_kernels_all", "medgp_profile_num_kernels_ext", "medgp_profile_num_kernels_ext2", "medgp_profile_num_kernels_ext3", "medgp_profile_kernel_name_ext3",
    "medgp_profile_kernel_name", "medgp_profile_read", "medgp_profile_reset", "medgp_kde_mode", "medgp_kde_mode_at", "medgp_gmm_fit",
]


class MedgpError(RuntimeError):
    pass


def lib_path():
    """The in-tree library; MEDGP_LIB selects another build of the SAME ABI (A/B measurements of kernel variants)."""
    return os.environ.get("MEDGP_LIB") or os.path.join(_HERE, "libmedgp_hip.so")


_lib = None


def load():
    """dlopen the HIP library; raises (never falls back) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise MedgpError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(make -C medgp_amd/csrc). medgp_amd has no CPU fallback.")
    # Share ONE HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's);
    # whichever is loaded first is used by both, and a torch initialised after a foreign runtime can come
    # up with "No HIP GPUs are available".  So when torch is importable, let it load first.  (The C ABI
    # itself has no torch dependency; C/C++ hosts are unaffected.)
    try:
        import torch  # noqa: F401
    except Exception:   # pragma: no cover
        pass
    lib = C.CDLL(p)
    vp, i32p, dp, fp, u8p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lib.medgp_abi_version.restype = C.c_int
    lib.medgp_device_count.restype = C.c_int
    lib.medgp_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.medgp_destroy.argtypes = [vp]
    lib.medgp_destroy.restype = None
    lib.medgp_last_error.argtypes = [vp]
    lib.medgp_last_error.restype = C.c_char_p
    lib.medgp_num_hyp.argtypes = [vp]
    lib.medgp_set_pi.argtypes = [vp, C.c_double]
    lib.medgp_set_stream.argtypes = [vp, vp]
    lib.medgp_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.medgp_reserve_plan.argtypes = [vp, C.c_int, i32p, C.c_int]
    lib.medgp_alloc_stats.argtypes = [vp, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.medgp_set_patient.argtypes = [vp, C.c_int, C.c_int, i32p, fp, fp]
    lib.medgp_set_patients.argtypes = [vp, C.c_int, i32p, C.POINTER(C.c_int64), i32p, fp, fp]
    lib.medgp_set_prior.argtypes = [vp, C.c_int, u8p, i32p, u8p, fp, fp]
    lib.medgp_set_priors.argtypes = [vp, C.c_int, i32p, u8p, i32p, u8p, fp, fp]
    lib.medgp_host_alloc.argtypes = [C.c_size_t]
    lib.medgp_host_alloc.restype = vp
    lib.medgp_host_free.argtypes = [vp]
    lib.medgp_host_free.restype = None
    lib.medgp_nlml_grad_async.argtypes = [vp, C.c_int, C.c_int, i32p, vp, C.c_int, vp, vp, vp]
    lib.medgp_wait.argtypes = [vp, C.c_int]
    lib.medgp_nlml_grad.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, i32p]
    lib.medgp_screen.argtypes = [vp, C.c_int, i32p, C.c_int, dp, dp, i32p]
    lib.medgp_nlml_grad_device.argtypes = [vp, C.c_int, i32p, vp, C.c_int, vp, vp, vp]
    lib.medgp_get_factor.argtypes = [vp, C.c_int, fp, fp, fp]
    lib.medgp_factor.argtypes = [vp, C.c_int, dp, dp, dp, i32p]
    lib.medgp_factor_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(dp), C.POINTER(dp), i32p]
    lib.medgp_pin_route.argtypes = [vp, C.c_int]
    lib.medgp_last_plan.argtypes = [vp, C.c_int, i32p, i32p, i32p]
    lib.medgp_fit_predict.argtypes = [vp, C.c_int, dp, C.c_int, i32p, fp, fp, fp, i32p]
    lib.medgp_fit_predict_batch.argtypes = [vp, C.c_int, i32p, dp, i32p, fp, fp, fp, i32p]
    lib.medgp_posterior_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, fp, fp, fp, i32p]
    lib.medgp_posterior_joint_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, C.c_int, dp, fp, fp, fp, fp, i32p, i32p]
    lib.medgp_loo_batch.argtypes = [vp, C.c_int, i32p, dp, i32p, i32p, fp, fp, dp, dp, i32p, i32p]
    lib.medgp_loo_grad.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, i32p]
    lib.medgp_lgo_grad.argtypes = [vp, C.c_int, i32p, dp, i32p, i32p, C.c_int, dp, dp, i32p, i32p]
    lib.medgp_fisher_vec.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, i32p]
    lib.medgp_hess_vec.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, dp, i32p]
    lib.medgp_posterior_jvp_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, C.c_int, dp, fp, fp, dp, dp, i32p]
    lib.medgp_posterior_vjp_batch.restype = C.c_int
    lib.medgp_posterior_vjp_moments.restype = C.c_int
    lib.medgp_posterior_vjp_moments.argtypes = [vp, C.c_int64, dp, dp]
    lib.medgp_mean_nlml_grad.restype = C.c_int
    lib.medgp_mean_nlml_grad.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, C.c_int, dp, dp, dp, dp, dp, i32p]
    lib.medgp_mean_posterior_batch.restype = C.c_int
    lib.medgp_mean_posterior_batch.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, C.POINTER(C.c_int64), i32p, fp, dp, dp, dp, i32p]
    lib.medgp_set_basis.restype = C.c_int
    lib.medgp_set_basis.argtypes = [vp, C.c_int, i32p, C.c_int, C.POINTER(C.c_int64), dp]
    lib.medgp_basis_nlml_grad.restype = C.c_int
    lib.medgp_basis_nlml_grad.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, C.c_int, dp, dp, dp, dp, dp, i32p]
    lib.medgp_basis_posterior_batch.restype = C.c_int
    lib.medgp_basis_posterior_batch.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, C.POINTER(C.c_int64), i32p, fp, dp, dp, dp, dp, i32p]
    lib.medgp_warp_nlml_grad.restype = C.c_int
    lib.medgp_warp_nlml_grad.argtypes = [vp, C.c_int, i32p, dp, i32p, dp, C.c_int, dp, dp, dp, dp, i32p]
    lib.medgp_warp_posterior_batch.restype = C.c_int
    lib.medgp_warp_posterior_batch.argtypes = [vp, C.c_int, i32p, dp, i32p, dp, C.POINTER(C.c_int64), i32p, fp, fp, C.c_int, dp, dp, dp, dp, dp, i32p]
    lib.medgp_set_noise_scale.restype = C.c_int
    lib.medgp_set_noise_scale.argtypes = [vp, C.c_int, i32p, C.POINTER(C.c_int64), dp]
    lib.medgp_hetero_nlml_grad.restype = C.c_int
    lib.medgp_hetero_nlml_grad.argtypes = [vp, C.c_int, i32p, dp, C.c_int, dp, dp, dp, dp, i32p]
    lib.medgp_hetero_posterior_batch.restype = C.c_int
    lib.medgp_hetero_posterior_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, dp, dp, dp, i32p]
    lib.medgp_robust_nlml_grad.restype = C.c_int
    lib.medgp_robust_nlml_grad.argtypes = [vp, C.c_int, i32p, dp, dp, C.c_int, dp, C.c_int, dp, dp, dp, dp, dp, dp, i32p]
    lib.medgp_profile_num_kernels_ext3.restype = C.c_int
    lib.medgp_profile_kernel_name_ext3.restype = C.c_char_p
    lib.medgp_profile_kernel_name_ext3.argtypes = [C.c_int]
    lib.medgp_posterior_vjp_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, C.c_int, dp, dp, C.c_int, dp, dp, fp, fp, dp, dp, i32p]
    lib.medgp_forecast_grad.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, C.c_int, dp, dp, i32p]
    lib.medgp_forecast_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, i32p, fp, fp, fp, dp, i32p]
    lib.medgp_trend_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, fp, fp, fp, fp, fp, i32p]
    lib.medgp_components_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), i32p, fp, fp, fp, fp, i32p]
    lib.medgp_functional_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32p, fp, dp, fp, fp, i32p]
    lib.medgp_functional_joint_batch.argtypes = [vp, C.c_int, i32p, dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), i32p, fp, dp, fp, fp, fp, i32p]
    lib.medgp_synchronize.argtypes = [vp]
    lib.medgp_profile_enable.argtypes = [vp, C.c_int]
    lib.medgp_profile_num_kernels.restype = C.c_int
    lib.medgp_profile_num_kernels_all.restype = C.c_int
    lib.medgp_profile_num_kernels_ext.restype = C.c_int
    lib.medgp_profile_num_kernels_ext2.restype = C.c_int
    lib.medgp_profile_kernel_name.argtypes = [C.c_int]
    lib.medgp_profile_kernel_name.restype = C.c_char_p
    lib.medgp_profile_read.argtypes = [vp, C.c_int, dp, C.POINTER(C.c_int64)]
    lib.medgp_profile_reset.argtypes = [vp]
    lib.medgp_kde_mode.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), i32p, dp, C.c_int, dp, dp, i32p, dp]
    lib.medgp_kde_mode_at.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int64), i32p, dp, C.POINTER(C.c_int64), i32p, dp, C.c_int, dp, dp, i32p, dp]
    lib.medgp_gmm_fit.argtypes = [C.c_int, C.c_int, C.c_int, dp, C.c_int, i32p, i32p, C.c_int, C.c_double, C.c_double, dp, dp, i32p, i32p,
                                  dp, dp, dp, i32p, dp]
    _lib = lib
    return lib


def _ptr(a, ty):
    return None if a is None else a.ctypes.data_as(C.POINTER(ty))


def _cat(arrs, M, dtype, tail=()):
    """the per-patient arrays of a call's M points as one array [M, *tail]; a call without points hands over one element that is never read"""
    return np.ascontiguousarray(np.concatenate(arrs, axis=0) if M else np.zeros((1,) + tuple(tail)), dtype=dtype)


def _split(offsets, *arrays):
    """per patient b the copies of rows [offsets[b], offsets[b + 1]) of every array, as a tuple; a None array stays None"""
    for a, e in zip(offsets[:-1], offsets[1:]):
        yield tuple(None if x is None else x[int(a):int(e)].copy() for x in arrays)


def _pack(series):
    ns = len(series)
    cnt = np.array([0 if x is None else np.size(x) for x in series], dtype=np.int32)
    off = np.zeros(ns, dtype=np.int64)
    if ns:
        off[1:] = np.cumsum(cnt[:-1], dtype=np.int64)
    parts = [np.asarray(x, dtype=np.float64).ravel() for x in series if x is not None]
    data = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0))
    return off, cnt, data


def kde_mode(series, weighted=True, device=0, full=False, test=None):
    """medgp_kde_mode[_at] over a list of 1-D sample arrays: the KDE "mode" of each (compute_kde + compute_mode of the
    reference, ref: medgpc/clustering/mode_estimate.py:438-450).  test: optional list (entries may be None) of evaluation
    grids, one per series -- the density is then evaluated there and the mode taken over the grid.  Returns modes
    [len(series)]; with full=True also (bandwidths, status, kernel milliseconds).  status -1 marks a series the reference's
    KDE fit raises on."""
    lib = load()
    ns = len(series)
    off, cnt, data = _pack(series)
    mode, bw, st, ms = np.full(ns, np.nan), np.full(ns, np.nan), np.zeros(ns, dtype=np.int32), C.c_double(0.0)
    if test is None:
        rc = lib.medgp_kde_mode(int(device), ns, _ptr(off, C.c_int64), _ptr(cnt, C.c_int32), _ptr(data, C.c_double),
                                1 if weighted else 0, _ptr(mode, C.c_double), _ptr(bw, C.c_double), _ptr(st, C.c_int32), C.byref(ms))
    else:
        assert len(test) == ns
        toff, tcnt, tdata = _pack(test)
        rc = lib.medgp_kde_mode_at(int(device), ns, _ptr(off, C.c_int64), _ptr(cnt, C.c_int32), _ptr(data, C.c_double),
                                   _ptr(toff, C.c_int64), _ptr(tcnt, C.c_int32), _ptr(tdata, C.c_double), 1 if weighted else 0,
                                   _ptr(mode, C.c_double), _ptr(bw, C.c_double), _ptr(st, C.c_int32), C.byref(ms))
    if rc != 0:
        raise MedgpError(f"medgp_kde_mode failed ({rc}): {lib.medgp_last_error(None).decode()}")
    return (mode, bw, st, ms.value) if full else mode


def gmm_fit(x, k, label0, max_iter=2000, tol=1e-3, reg_covar=1e-6, device=0, full=False):
    """medgp_gmm_fit: EM for full-covariance Gaussian mixtures on the points x [n, d], len(k) independent runs in one call; run r has
    k[r] components and starts from the hard labels label0[r] [n] (what scikit-learn's GaussianMixture.fit does from its k-means
    start inside the reference's run_sklearn_gmm, ref: medgpc/clustering/cluster.py:23-46).  Returns (lower_bound, bic, n_iter,
    status) per run -- status 1 converged, 0 max_iter reached, -1 failed (NaN lower_bound / bic) -- and with full=True also (weights
    [nruns, kmax], means [nruns, kmax, d], covs [nruns, kmax, d, d], assign [nruns, n], kernel milliseconds)."""
    lib = load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2:
        raise ValueError(f"x of shape {x.shape}, expected [n, d]")
    n, d = x.shape
    k = np.ascontiguousarray(np.atleast_1d(k), dtype=np.int32)
    nr = k.shape[0]
    label0 = np.ascontiguousarray(label0, dtype=np.int32)
    if k.ndim != 1 or nr < 1 or label0.size != nr * n:
        raise ValueError(f"{label0.size} start labels for {nr} runs of {n} points")
    kmax = max(int(k.max()), 1)
    lb, bic = np.full(nr, np.nan), np.full(nr, np.nan)
    nit, st = np.zeros(nr, dtype=np.int32), np.zeros(nr, dtype=np.int32)
    w = mu = cv = asg = None
    ms = C.c_double(0.0)
    if full:
        w, mu, cv = np.zeros((nr, kmax)), np.zeros((nr, kmax, d)), np.zeros((nr, kmax, d, d))
        asg = np.zeros((nr, n), dtype=np.int32)
    rc = lib.medgp_gmm_fit(int(device), n, d, _ptr(x, C.c_double), nr, _ptr(k, C.c_int32), _ptr(label0, C.c_int32), int(max_iter),
                           float(tol), float(reg_covar), _ptr(lb, C.c_double), _ptr(bic, C.c_double), _ptr(nit, C.c_int32),
                           _ptr(st, C.c_int32), _ptr(w, C.c_double), _ptr(mu, C.c_double), _ptr(cv, C.c_double), _ptr(asg, C.c_int32),
                           C.byref(ms))
    if rc != 0:
        err = MedgpError(f"medgp_gmm_fit failed ({rc}): {lib.medgp_last_error(None).decode()}")
        err.code = rc
        raise err
    return (lb, bic, nit, st, w, mu, cv, asg, ms.value) if full else (lb, bic, nit, st)


class Context:
    """One (device, covariance family) evaluation context."""

    def __init__(self, kernel_index=KERNEL_LMC_SM, Q=5, D=2, R=2, device=0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.medgp_create(C.byref(h), int(device), int(kernel_index), int(Q), int(D), int(R))
        if rc != 0:
            raise MedgpError(f"medgp_create failed ({rc}): {self._lib.medgp_last_error(None).decode()}")
        self._h = h
        self.kernel_index, self.Q, self.D, self.R, self.device = kernel_index, Q, D, R, device
        self.H = self._lib.medgp_num_hyp(h)
        self._slot_n, self._slot_meta = {}, {}   # n and meta of the patient in each slot (loo() lays out its outputs by them)

    def _chk(self, rc):
        if rc != 0:
            raise MedgpError(f"libmedgp_hip error {rc}: {self._lib.medgp_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.medgp_destroy(self._h)
            self._h = None
            self._lane_refs = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_pi(self, pi):
        self._chk(self._lib.medgp_set_pi(self._h, float(pi)))

    def set_stream(self, stream_ptr):
        self._chk(self._lib.medgp_set_stream(self._h, C.c_void_p(stream_ptr or 0)))

    def reserve(self, max_slots, max_n, max_batch):
        self._chk(self._lib.medgp_reserve(self._h, int(max_slots), int(max_n), int(max_batch)))

    def reserve_plan(self, sizes, ninit=0):
        """medgp_reserve_plan: announce the sizes of the patients that will be resident together (and the width of the screening):
        the per-entry arenas are allocated once to what the largest call over them needs."""
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        self._chk(self._lib.medgp_reserve_plan(self._h, int(sizes.shape[0]), _ptr(sizes, C.c_int32), int(ninit)))

    def alloc_stats(self):
        """(seconds spent in device-memory management calls, number of such calls, bytes held by the per-entry arenas)"""
        s, n, b = C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        self._chk(self._lib.medgp_alloc_stats(self._h, C.byref(s), C.byref(n), C.byref(b)))
        return s.value, n.value, b.value

    def set_patient(self, slot, meta, t, y):
        t = np.ascontiguousarray(t, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        meta = None if meta is None else np.ascontiguousarray(meta, dtype=np.int32)
        self._chk(self._lib.medgp_set_patient(self._h, int(slot), int(t.shape[0]), _ptr(meta, C.c_int32),
                                              _ptr(t, C.c_float), _ptr(y, C.c_float)))
        self._remember(int(slot), meta, int(t.shape[0]))

    def _remember(self, slot, meta, n):
        self._slot_n[slot] = n
        self._slot_meta[slot] = None if meta is None else np.array(meta, dtype=np.int32)

    def set_patients(self, slots, patients):
        """Packed upload: patients = list of (meta, t, y); one H2D transfer, no device wait."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        ns = [np.asarray(p[1]).shape[0] for p in patients]
        offsets = np.zeros(len(ns) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(ns)
        t = np.ascontiguousarray(np.concatenate([np.asarray(p[1], dtype=np.float32) for p in patients]), dtype=np.float32)
        y = np.ascontiguousarray(np.concatenate([np.asarray(p[2], dtype=np.float32) for p in patients]), dtype=np.float32)
        meta = None
        if patients[0][0] is not None:
            meta = np.ascontiguousarray(np.concatenate([np.asarray(p[0], dtype=np.int32) for p in patients]), dtype=np.int32)
        self._chk(self._lib.medgp_set_patients(self._h, len(ns), _ptr(slots, C.c_int32), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                               _ptr(meta, C.c_int32), _ptr(t, C.c_float), _ptr(y, C.c_float)))
        for s, p in zip(slots, patients):
            self._remember(int(s), p[0], int(np.asarray(p[1]).shape[0]))

    def set_prior(self, slot, flag=None, type=None, is_exp=None, p0=None, p1=None):
        if flag is None:
            self._chk(self._lib.medgp_set_prior(self._h, int(slot), None, None, None, None, None))
            return
        flag = np.ascontiguousarray(flag, dtype=np.uint8)
        type = np.ascontiguousarray(type, dtype=np.int32)
        is_exp = np.ascontiguousarray(is_exp, dtype=np.uint8)
        p0 = np.ascontiguousarray(p0, dtype=np.float32)
        p1 = np.ascontiguousarray(p1, dtype=np.float32)
        assert flag.shape[0] == self.H
        self._chk(self._lib.medgp_set_prior(self._h, int(slot), _ptr(flag, C.c_uint8), _ptr(type, C.c_int32),
                                            _ptr(is_exp, C.c_uint8), _ptr(p0, C.c_float), _ptr(p1, C.c_float)))

    def set_priors(self, slots, flag=None, type=None, is_exp=None, p0=None, p1=None):
        """Batched medgp_set_prior: arrays are [len(slots), H]; one transfer, no device wait."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        ns = slots.shape[0]
        if flag is None:
            self._chk(self._lib.medgp_set_priors(self._h, ns, _ptr(slots, C.c_int32), None, None, None, None, None))
            return
        arrs = [np.ascontiguousarray(a, dtype=dt).reshape(ns, self.H) for a, dt in
                ((flag, np.uint8), (type, np.int32), (is_exp, np.uint8), (p0, np.float32), (p1, np.float32))]
        self._chk(self._lib.medgp_set_priors(self._h, ns, _ptr(slots, C.c_int32), _ptr(arrs[0], C.c_uint8), _ptr(arrs[1], C.c_int32),
                                             _ptr(arrs[2], C.c_uint8), _ptr(arrs[3], C.c_float), _ptr(arrs[4], C.c_float)))

    def pinned(self, shape, dtype):
        """numpy array in pinned host memory (medgp_host_alloc).  The memory belongs to the ARRAY, not to the context: it is
        freed (medgp_host_free) when the last view of it is garbage collected, so an array a caller still holds after close()
        stays valid.  Arrays handed to nlml_grad_async are additionally kept alive by the context until wait(lane)."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self._lib.medgp_host_alloc(max(n, 1))
        if not p:
            raise MedgpError("medgp_host_alloc failed")
        buf = (C.c_char * max(n, 1)).from_address(p)
        weakref.finalize(buf, self._lib.medgp_host_free, p)   # every numpy view keeps `buf` alive through its .base chain
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def nlml_grad_async(self, lane, slots, theta, flag_grad, nlml, grad, status):
        """medgp_nlml_grad_async: theta / nlml / grad / status are (pinned) numpy arrays that stay alive until wait(lane)."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        if not hasattr(self, "_lane_refs"):
            self._lane_refs = {}
        self._lane_refs[int(lane)] = (theta, nlml, grad, status)   # the device writes into these until wait(lane)
        self._chk(self._lib.medgp_nlml_grad_async(self._h, int(lane), slots.shape[0], _ptr(slots, C.c_int32),
                                                  C.c_void_p(theta.ctypes.data), int(bool(flag_grad)), C.c_void_p(nlml.ctypes.data),
                                                  C.c_void_p(grad.ctypes.data if grad is not None else 0),
                                                  C.c_void_p(status.ctypes.data if status is not None else 0)))

    def wait(self, lane):
        self._chk(self._lib.medgp_wait(self._h, int(lane)))
        getattr(self, "_lane_refs", {}).pop(int(lane), None)

    def pin_route(self, pinned=True):
        """medgp_pin_route: one factorisation kernel for every call, so a patient's bits do not depend on its batch-mates."""
        self._chk(self._lib.medgp_pin_route(self._h, 1 if pinned else 0))

    def screen(self, slots, theta):
        """medgp_screen: the hyper vectors theta [ninit, H] evaluated (nlml only) on every patient of slots. Returns (nlml, status),
        both [len(slots), ninit]."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1, self.H)
        ns, ni = slots.shape[0], theta.shape[0]
        nlml = np.empty((ns, ni), dtype=np.float64)
        st = np.empty((ns, ni), dtype=np.int32)
        self._chk(self._lib.medgp_screen(self._h, ns, _ptr(slots, C.c_int32), ni, _ptr(theta, C.c_double), _ptr(nlml, C.c_double), _ptr(st, C.c_int32)))
        return nlml, st

    def last_plan(self):
        """medgp_last_plan: [(entries, 64-blocks of the largest, route)] of the last nlml_grad call's size classes, largest first;
        route 0 / 1 = one workgroup per entry (4- / 8-wave shape), 2 = multi-CU look-ahead schedule."""
        cnt, blk, rt = (np.zeros(32, np.int32) for _ in range(3))
        nc = self._lib.medgp_last_plan(self._h, 32, _ptr(cnt, C.c_int32), _ptr(blk, C.c_int32), _ptr(rt, C.c_int32))
        if nc < 0:
            self._chk(nc)
        return [(int(cnt[i]), int(blk[i]), int(rt[i])) for i in range(min(nc, 32))]

    def nlml_grad(self, slots, theta, flag_grad=True, keep_factor=False):
        """Host-pointer operator. theta: [nbatch, H]. Returns (nlml[nbatch], grad[nbatch,H] or None, status[nbatch]).
        keep_factor: MEDGP_FLAG_KEEP_FACTOR (alpha / L^-1 available through get_factor even without gradients)."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        nlml = np.empty(nb)
        grad = np.empty((nb, self.H)) if flag_grad else None
        status = np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_nlml_grad(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double),
                                            int(bool(flag_grad)) | (FLAG_KEEP_FACTOR if keep_factor else 0),
                                            _ptr(nlml, C.c_double), _ptr(grad, C.c_double), _ptr(status, C.c_int32)))
        return nlml, grad, status

    def nlml_grad_device(self, slots, theta_ptr, flag_grad, nlml_ptr, grad_ptr, status_ptr):
        """Device-pointer operator (asynchronous on the context's stream). Pointers are integers (tensor.data_ptr())."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        self._chk(self._lib.medgp_nlml_grad_device(self._h, slots.shape[0], _ptr(slots, C.c_int32), C.c_void_p(theta_ptr),
                                                   int(bool(flag_grad)), C.c_void_p(nlml_ptr), C.c_void_p(grad_ptr or 0),
                                                   C.c_void_p(status_ptr or 0)))

    def get_factor(self, b, n, want_linv=True):
        alpha = np.empty(n, dtype=np.float32)
        linv = np.empty((n, n), dtype=np.float32) if want_linv else None
        beta = C.c_float()
        self._chk(self._lib.medgp_get_factor(self._h, int(b), _ptr(alpha, C.c_float), _ptr(linv, C.c_float), C.byref(beta)))
        return alpha, linv, beta.value

    def factor(self, slot, theta, n):
        """Cholesky factor (caller order, lower, fp64) and z = L^-1 y of one patient. Returns (L[n,n], z[n], status)."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        Lm = np.zeros((n, n))
        z = np.zeros(n)
        st = C.c_int32()
        self._chk(self._lib.medgp_factor(self._h, int(slot), _ptr(theta, C.c_double), _ptr(Lm, C.c_double), _ptr(z, C.c_double), C.byref(st)))
        return Lm, z, st.value

    def factor_batch(self, slots, theta, ns):
        """medgp_factor_batch: list of (L[n,n], z[n]) per entry and the status array; ns = observations of each entry."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        Ls = [np.zeros((int(n), int(n))) for n in ns]
        zs = [np.zeros(int(n)) for n in ns]
        Lp = (C.POINTER(C.c_double) * nb)(*[_ptr(a, C.c_double) for a in Ls])
        zp = (C.POINTER(C.c_double) * nb)(*[_ptr(a, C.c_double) for a in zs])
        st = np.zeros(nb, dtype=np.int32)
        self._chk(self._lib.medgp_factor_batch(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), Lp, zp, _ptr(st, C.c_int32)))
        return list(zip(Ls, zs)), st

    def fit_predict(self, slot, theta, meta2, t2):
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        t2 = np.ascontiguousarray(t2, dtype=np.float32)
        meta2 = None if meta2 is None else np.ascontiguousarray(meta2, dtype=np.int32)
        ns = t2.shape[0]
        mean = np.empty(ns, dtype=np.float32)
        var = np.empty(ns, dtype=np.float32)
        st = C.c_int32()
        self._chk(self._lib.medgp_fit_predict(self._h, int(slot), _ptr(theta, C.c_double), ns, _ptr(meta2, C.c_int32),
                                              _ptr(t2, C.c_float), _ptr(mean, C.c_float), _ptr(var, C.c_float), C.byref(st)))
        return mean, var, st.value

    def fit_predict_batch(self, slots, theta, meta2, t2):
        """One test point per problem: problem b = (slots[b], theta[b], meta2[b], t2[b])."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        t2 = np.ascontiguousarray(t2, dtype=np.float32)
        meta2 = None if meta2 is None else np.ascontiguousarray(meta2, dtype=np.int32)
        mean = np.empty(nb, dtype=np.float32)
        var = np.empty(nb, dtype=np.float32)
        st = np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_fit_predict_batch(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double),
                                                    _ptr(meta2, C.c_int32), _ptr(t2, C.c_float), _ptr(mean, C.c_float),
                                                    _ptr(var, C.c_float), _ptr(st, C.c_int32)))
        return mean, var, st

    def _batch_args(self, slots, theta, check=False):
        """(slots int32 [nbatch], theta float64 [nbatch, H]) as every batched call takes them; check: a theta of another size is
        refused in the wrappers' own words instead of numpy's"""
        slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        nb = slots.shape[0]
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if check and theta.size != nb * self.H:
            raise ValueError(f"theta has {theta.size} values, expected {nb} x {self.H}")
        return slots, theta.reshape(nb, self.H)

    def _point_args(self, slots, theta, meta2_list, t2_list):
        """The one pack of a call that takes test points, after its argument checks: slots, theta [nbatch, H]; ms / ts the covariate
        and time arrays per patient; cnt, offsets [nbatch + 1] and M = the points per patient, their CSR and their number; m2 / t2 the
        concatenated arrays (one never-read element when M = 0); head = (handle, nbatch, slots, theta) and pts = (offsets, meta2, t2)
        as the C calls take them."""
        slots, theta = self._batch_args(slots, theta, check=True)
        nb = slots.shape[0]
        if len(t2_list) != nb:
            raise ValueError(f"{len(t2_list)} test-point arrays for {nb} patients")
        ts = [np.ascontiguousarray(x, dtype=np.float32).ravel() for x in t2_list]
        if meta2_list is None:
            if self.kernel_index == KERNEL_LMC_SM:
                raise ValueError("meta2_list is required for the multi-output kernel")
            ms = [np.zeros(x.shape[0], dtype=np.int32) for x in ts]
        else:
            if len(meta2_list) != nb:
                raise ValueError(f"{len(meta2_list)} covariate arrays for {nb} patients")
            ms = [np.ascontiguousarray(x, dtype=np.int32).ravel() for x in meta2_list]
            for b, (m, x) in enumerate(zip(ms, ts)):
                if m.shape[0] != x.shape[0]:
                    raise ValueError(f"patient {b}: {m.shape[0]} covariates for {x.shape[0]} test times")
        cnt = np.array([x.shape[0] for x in ts], dtype=np.int64)
        offsets = np.zeros(nb + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(cnt)
        M = int(offsets[-1])
        p = SimpleNamespace(slots=slots, theta=theta, nb=nb, ms=ms, ts=ts, cnt=cnt, offsets=offsets, M=M, Mz=max(M, 1),
                            t2=_cat(ts, M, np.float32), m2=_cat(ms, M, np.int32), st=np.empty(nb, dtype=np.int32))
        p.head = (self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double))
        p.pts = (_ptr(offsets, C.c_int64), _ptr(p.m2, C.c_int32), _ptr(p.t2, C.c_float))
        return p

    @staticmethod
    def _per_point(p, lst, dtype, what, width=None):
        """one array per patient, matching the t2_list of the pack p, as one array of dtype: [M] of arrays [m] (width None), [M, width]
        of arrays [m, width] (or anything of m x width values); a None list stays None"""
        if lst is None:
            return None
        if len(lst) != p.nb:
            raise ValueError(f"{len(lst)} {what} arrays for {p.nb} patients")
        tail = () if width is None else (width,)
        rows = [np.ascontiguousarray(x, dtype=dtype) for x in lst]
        for b, (a, m) in enumerate(zip(rows, p.cnt)):
            if a.size != m * (1 if width is None else width):
                raise ValueError(f"patient {b}: {what} of shape {a.shape} for {int(m)} test points, expected {(int(m),) + tail}")
        return _cat([a.reshape((int(m),) + tail) for a, m in zip(rows, p.cnt)], p.M, dtype, tail)

    def posterior(self, slots, theta, meta2_list, t2_list, parts=True):
        """medgp_posterior_batch: GP_Regression::predict / parsed_predict for many points of many patients in one call.
        slots [nbatch], theta [nbatch, H]; t2_list: one array of test times per patient (may be empty), meta2_list: one array of
        test covariates per patient (None for SE / SM).  Returns ([(mean[m], var[m], parts[m, D] or None) per patient], status)."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        D = self.D if self.kernel_index == KERNEL_LMC_SM else 1
        mean, var = (np.empty(p.Mz, dtype=np.float32) for _ in range(2))
        pr = np.empty((p.Mz, D), dtype=np.float32) if parts else None
        self._chk(self._lib.medgp_posterior_batch(*p.head, *p.pts, _ptr(mean, C.c_float), _ptr(var, C.c_float), _ptr(pr, C.c_float),
                                                  _ptr(p.st, C.c_int32)))
        return list(_split(p.offsets, mean, var, pr)), p.st

    def forecast(self, slots, theta, meta2_list, t2_list, prefix_list=None, y2_list=None):
        """medgp_forecast_batch: point j of patient b predicted from the FIRST prefix_list[b][j] observations of the patient in the
        order they were uploaded (rolling-origin forecasts when that is time order; medgp_amd.forecast.rolling_origin builds the
        points).  slots, theta, meta2_list, t2_list as posterior(); prefix_list: one int array per patient, values in [0, n_b]
        (None: all of the patient's data); y2_list: the observed values at the points (None: no lpd).
        Returns ([(mean[m], var[m], lpd[m] or None) per patient], status)."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        pf = self._per_point(p, prefix_list, np.int32, "prefix")
        y2 = self._per_point(p, y2_list, np.float32, "y2")
        mean, var = (np.empty(p.Mz, dtype=np.float32) for _ in range(2))
        lpd = np.empty(p.Mz, dtype=np.float64) if y2 is not None else None
        self._chk(self._lib.medgp_forecast_batch(*p.head, *p.pts, _ptr(pf, C.c_int32), _ptr(y2, C.c_float), _ptr(mean, C.c_float),
                                                 _ptr(var, C.c_float), _ptr(lpd, C.c_double), _ptr(p.st, C.c_int32)))
        return list(_split(p.offsets, mean, var, lpd)), p.st

    def trend(self, slots, theta, meta2_list, t2_list, cross=True):
        """medgp_trend_batch: the posterior of the latent slope f'(t*) at every test point, next to the posterior of the value.
        Arguments as posterior().  Returns ([(mean[m], var[m], dmean[m], dvar[m], cross[m] or None) per patient], status): mean /
        var are posterior(parts=False)'s, bit for bit; dmean is the slope per hour in the units of y, dvar the variance of the
        LATENT slope (no noise term), cross = cov(f(t*), f'(t*)).  medgp_amd.trend turns them into P(rising) and rate intervals."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        mean, var, dmean, dvar = (np.empty(p.Mz, dtype=np.float32) for _ in range(4))
        cr = np.empty(p.Mz, dtype=np.float32) if cross else None
        self._chk(self._lib.medgp_trend_batch(*p.head, *p.pts, _ptr(mean, C.c_float), _ptr(var, C.c_float), _ptr(dmean, C.c_float),
                                              _ptr(dvar, C.c_float), _ptr(cr, C.c_float), _ptr(p.st, C.c_int32)))
        return list(_split(p.offsets, mean, var, dmean, dvar, cr)), p.st

    def components(self, slots, theta, meta2_list, t2_list, cov=True):
        """medgp_components_batch: the posterior of every spectral component f_q of the latent f = sum_q f_q at every test point.
        Arguments as posterior().  Returns ([(cmean[m, Q], cvar[m, Q], ccov[m, Q, Q] or None) per patient], status): cmean[j, q] the
        posterior mean of f_q at point j, ccov[j] the Q x Q posterior covariance of the components there (LATENT: no noise term),
        cvar[j] its diagonal.  medgp_amd.components names the components (period, length scale, weight) and sums bands of them."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        Q = self.Q
        cmean, cvar = (np.empty((p.Mz, Q), dtype=np.float32) for _ in range(2))
        cc = np.empty((p.Mz, Q, Q), dtype=np.float32) if cov else None
        self._chk(self._lib.medgp_components_batch(*p.head, *p.pts, _ptr(cmean, C.c_float), _ptr(cvar, C.c_float), _ptr(cc, C.c_float),
                                                   _ptr(p.st, C.c_int32)))
        return list(_split(p.offsets, cmean, cvar, cc)), p.st

    def functionals(self, slots, theta, packed_list):
        """medgp_functional_batch: the posterior of linear functionals g = sum_k a_k f_{m_k}(t_k) of the latent function -- window
        means, change scores, contrasts (medgp_amd.functionals builds and packs them).  slots [nbatch], theta [nbatch, H];
        packed_list: per patient (toffsets [F + 1], meta2 [T] or None for SE / SM, t2 [T], weight [T]) as functionals.pack returns
        it; a patient may have no functionals, a functional no terms.  Returns ([(fmean[F], fvar[F]) per patient], status): the
        posterior mean and the LATENT posterior variance (no noise term, no clamp) of every functional."""
        slots, theta, foffsets, toffsets, m2, t2, wt = self._functional_args(slots, theta, packed_list)
        nb, F = slots.shape[0], int(foffsets[-1])
        fmean, fvar = (np.empty(max(F, 1), dtype=np.float32) for _ in range(2))
        st = np.empty(nb, dtype=np.int32)
        i64p = C.POINTER(C.c_int64)
        self._chk(self._lib.medgp_functional_batch(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double),
                                                   foffsets.ctypes.data_as(i64p), toffsets.ctypes.data_as(i64p), _ptr(m2, C.c_int32),
                                                   _ptr(t2, C.c_float), _ptr(wt, C.c_double), _ptr(fmean, C.c_float), _ptr(fvar, C.c_float),
                                                   _ptr(st, C.c_int32)))
        return list(_split(foffsets, fmean, fvar)), st

    def functionals_joint(self, slots, theta, packed_list):
        """medgp_functional_joint_batch: functionals() plus the posterior covariance between the functionals of each patient.
        Arguments and argument checks as functionals().  Returns ([(fmean[F], fvar[F], fcov[F, F]) per patient], status): fmean and
        fvar are functionals()' outputs bit for bit; fcov is LATENT (no noise term, no clamp), exactly symmetric, and its diagonal has
        the bits of fvar.  medgp_amd.design works on fcov (expected variance reduction of a measurement, greedy picks)."""
        slots, theta, foffsets, toffsets, m2, t2, wt = self._functional_args(slots, theta, packed_list)
        nb, F = slots.shape[0], int(foffsets[-1])
        cnt = np.diff(foffsets)
        coff = np.zeros(nb + 1, dtype=np.int64)
        coff[1:] = np.cumsum(cnt * cnt)
        fmean, fvar = (np.empty(max(F, 1), dtype=np.float32) for _ in range(2))
        fcov = np.empty(max(int(coff[-1]), 1), dtype=np.float32)
        st = np.empty(nb, dtype=np.int32)
        i64p = C.POINTER(C.c_int64)
        self._chk(self._lib.medgp_functional_joint_batch(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double),
                                                         foffsets.ctypes.data_as(i64p), toffsets.ctypes.data_as(i64p), _ptr(m2, C.c_int32),
                                                         _ptr(t2, C.c_float), _ptr(wt, C.c_double), _ptr(fmean, C.c_float),
                                                         _ptr(fvar, C.c_float), _ptr(fcov, C.c_float), _ptr(st, C.c_int32)))
        blocks = [fcov[int(coff[b]):int(coff[b + 1])].reshape(int(k), int(k)).copy() for b, k in enumerate(cnt)]
        return [mv + (c,) for mv, c in zip(_split(foffsets, fmean, fvar), blocks)], st

    def _functional_args(self, slots, theta, packed_list):
        """the argument checks of functionals() / functionals_joint(), raised before the library is reached: (slots, theta [nbatch, H],
        foffsets [nbatch + 1], toffsets [F + 1], meta2, t2, weight per term) as the calls take them"""
        slots, theta = self._batch_args(slots, theta, check=True)
        nb = slots.shape[0]
        if len(packed_list) != nb:
            raise ValueError(f"{len(packed_list)} packed functional lists for {nb} patients")
        multi = self.kernel_index == KERNEL_LMC_SM
        toffs, ms, ts, ws = [], [], [], []
        for b, pk in enumerate(packed_list):
            if len(pk) != 4:
                raise ValueError(f"patient {b}: expected (toffsets, meta2, t2, weight)")
            to = np.ascontiguousarray(pk[0], dtype=np.int64).ravel()
            t = np.ascontiguousarray(pk[2], dtype=np.float32).ravel()
            a = np.ascontiguousarray(pk[3], dtype=np.float64).ravel()
            if pk[1] is None:
                if multi:
                    raise ValueError("meta2 is required for the multi-output kernel")
                m = np.zeros(t.shape[0], dtype=np.int32)
            else:
                m = np.ascontiguousarray(pk[1], dtype=np.int32).ravel()
            if to.shape[0] < 1 or to[0] != 0 or np.any(np.diff(to) < 0):
                raise ValueError(f"patient {b}: toffsets must start at 0 and not decrease")
            if not (m.shape[0] == t.shape[0] == a.shape[0] == int(to[-1])):
                raise ValueError(f"patient {b}: {m.shape[0]} covariates, {t.shape[0]} times and {a.shape[0]} weights for {int(to[-1])} terms")
            if multi and m.size and (m.min() < 0 or m.max() >= self.D):
                raise ValueError(f"patient {b}: meta2 outside [0, {self.D})")
            toffs.append(to)
            ms.append(m)
            ts.append(t)
            ws.append(a)
        foffsets = np.zeros(nb + 1, dtype=np.int64)
        foffsets[1:] = np.cumsum([x.shape[0] - 1 for x in toffs])
        tbase = np.concatenate([[0], np.cumsum([int(x[-1]) for x in toffs])]).astype(np.int64)
        toffsets = np.ascontiguousarray(np.concatenate([[0]] + [x[1:] + tbase[b] for b, x in enumerate(toffs)]), dtype=np.int64)
        T = int(tbase[-1])
        return slots, theta, foffsets, toffsets, _cat(ms, T, np.int32), _cat(ts, T, np.float32), _cat(ws, T, np.float64)

    def posterior_joint(self, slots, theta, meta2_list, t2_list, eps_list=None, cov=True):
        """medgp_posterior_joint_batch: the joint predictive distribution of every patient's test points.  Arguments as
        posterior(); eps_list: one (m_b, nsamp) array of standard normals per patient (the caller's draws; the same nsamp for
        all), or None for the covariance only; cov=False: samples only.  Returns ([(mean[m], var[m], cov[m, m] or None,
        samples[m, nsamp] or None) per patient], status, cov_status): cov = K** - V^T V + diag(sigma^2), whose diagonal is var;
        samples[:, s] = mean + chol(cov) eps[:, s]."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        nb, ts, cnt = p.nb, p.ts, p.cnt
        nsamp = 0
        es = None
        if eps_list is None:
            if not cov:
                raise ValueError("neither cov nor samples asked for (eps_list is None and cov is False)")
        else:
            if len(eps_list) != nb:
                raise ValueError(f"{len(eps_list)} eps arrays for {nb} patients")
            es = [np.ascontiguousarray(x, dtype=np.float64) for x in eps_list]
            for b, (e, x) in enumerate(zip(es, ts)):
                if e.ndim != 2 or e.shape[0] != x.shape[0]:
                    raise ValueError(f"patient {b}: eps of shape {e.shape} for {x.shape[0]} test points, expected (m, nsamp)")
            widths = {e.shape[1] for e in es}
            if len(widths) != 1:
                raise ValueError(f"eps arrays of different nsamp: {sorted(widths)}")
            nsamp = widths.pop()
            if nsamp < 1:
                raise ValueError("eps arrays with nsamp = 0: pass eps_list=None for the covariance only")
        coff = np.zeros(nb + 1, dtype=np.int64)
        coff[1:] = np.cumsum(cnt * cnt)
        mean, var = (np.empty(p.Mz, dtype=np.float32) for _ in range(2))
        cv = np.empty(max(int(coff[-1]), 1), dtype=np.float32) if cov else None
        eps = sm = None
        if nsamp:
            eps = _cat(es, p.M, np.float64, (nsamp,))
            sm = np.empty((p.Mz, nsamp), dtype=np.float32)
        cst = np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_posterior_joint_batch(*p.head, *p.pts, int(nsamp), _ptr(eps, C.c_double), _ptr(mean, C.c_float),
                                                        _ptr(var, C.c_float), _ptr(cv, C.c_float), _ptr(sm, C.c_float), _ptr(p.st, C.c_int32),
                                                        _ptr(cst, C.c_int32)))
        blocks = [cv[int(coff[b]):int(coff[b + 1])].reshape(int(m), int(m)).copy() if cov else None for b, m in enumerate(cnt)]
        return [(mu, v, c, s) for (mu, v, s), c in zip(_split(p.offsets, mean, var, sm), blocks)], p.st, cst

    def _loo_args(self, slots, theta, groups):
        """the argument checks of loo(): (slots, theta [nbatch, H], observation counts, group ids or None, groups per patient or
        None); the observation counts and covariates of the patients are those set_patient[s] saw."""
        if np.size(slots) < 1:
            raise ValueError("no patient")
        slots, theta = self._batch_args(slots, theta, check=True)
        nb = slots.shape[0]
        missing = [int(s) for s in slots if int(s) not in self._slot_n]
        if missing:
            raise ValueError(f"slots {missing} hold no patient set through this Context")
        ns = [self._slot_n[int(s)] for s in slots]
        if groups is None:
            return slots, theta, ns, None, None
        if isinstance(groups, str):
            if groups != "covariate":
                raise ValueError(f"groups = {groups!r}: expected a list of int arrays, None or 'covariate'")
            D = self.D if self.kernel_index == KERNEL_LMC_SM else 1
            metas = [self._slot_meta[int(s)] for s in slots]
            gs = [np.zeros(n, dtype=np.int32) if m is None else np.ascontiguousarray(m, dtype=np.int32).ravel() for m, n in zip(metas, ns)]
            ng = np.full(nb, D, dtype=np.int32)
        else:
            if len(groups) != nb:
                raise ValueError(f"{len(groups)} group arrays for {nb} patients")
            gs = []
            for b, x in enumerate(groups):
                x = np.asarray(x)
                if x.size and not np.issubdtype(x.dtype, np.integer):
                    raise ValueError(f"patient {b}: group ids of dtype {x.dtype}, expected integers")
                gs.append(np.ascontiguousarray(x, dtype=np.int32).ravel())
            ng = np.array([int(x.max()) + 1 if x.size and x.max() >= 0 else 0 for x in gs], dtype=np.int32)
        for b, (x, n) in enumerate(zip(gs, ns)):
            if x.shape[0] != n:
                raise ValueError(f"patient {b}: {x.shape[0]} group ids for {n} observations")
            if x.size and (x.min() < -1 or x.max() >= ng[b]):
                raise ValueError(f"patient {b}: group ids outside [-1, {int(ng[b])})")
        return slots, theta, ns, gs, ng

    def loo(self, slots, theta, groups=None):
        """medgp_loo_batch: the leave-one-out / leave-group-out predictive distribution of the patients' own observations.
        slots [nbatch], theta [nbatch, H]; groups: None (every observation its own group: classic LOO), a list of one int array
        of group ids per patient (-1: never held out; the number of groups of a patient is its largest id + 1) or "covariate"
        (each patient's meta: leave-one-covariate-out, D groups).  Returns ([(mean[n], var[n], lpd[G], total) per patient],
        status, [group_status[G] per patient]): mean / var of y_i given the observations outside i's group, lpd the joint log
        density of each group's held-out values, total their sum (the log pseudo-likelihood)."""
        slots, theta, ns, gs, ng = self._loo_args(slots, theta, groups)
        nb = slots.shape[0]
        Gs = np.array(ns if gs is None else ng, dtype=np.int64)
        ooff = np.zeros(nb + 1, dtype=np.int64)
        ooff[1:] = np.cumsum(ns)
        goff = np.zeros(nb + 1, dtype=np.int64)
        goff[1:] = np.cumsum(Gs)
        NO, NG = int(ooff[-1]), int(goff[-1])
        grp = None if gs is None else np.ascontiguousarray(np.concatenate(gs) if NO else np.zeros(1), dtype=np.int32)
        mean = np.empty(max(NO, 1), dtype=np.float32)
        var = np.empty(max(NO, 1), dtype=np.float32)
        lpd = np.empty(max(NG, 1), dtype=np.float64)
        tot = np.empty(nb, dtype=np.float64)
        st = np.empty(nb, dtype=np.int32)
        gst = np.empty(max(NG, 1), dtype=np.int32)
        self._chk(self._lib.medgp_loo_batch(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), _ptr(grp, C.c_int32),
                                            _ptr(ng, C.c_int32), _ptr(mean, C.c_float), _ptr(var, C.c_float), _ptr(lpd, C.c_double),
                                            _ptr(tot, C.c_double), _ptr(st, C.c_int32), _ptr(gst, C.c_int32)))
        out, gstat = [], []
        for b in range(nb):
            a, e, ga, ge = int(ooff[b]), int(ooff[b + 1]), int(goff[b]), int(goff[b + 1])
            out.append((mean[a:e].copy(), var[a:e].copy(), lpd[ga:ge].copy(), float(tot[b])))
            gstat.append(gst[ga:ge].copy())
        return out, st, gstat

    def loo_grad(self, slots, theta, flag_grad=True):
        """medgp_loo_grad: the negative leave-one-out log pseudo-likelihood (plus the prior term, as nlml_grad) and its gradient
        in theta.  slots [nbatch], theta [nbatch, H].  Returns (obj[nbatch], grad[nbatch, H] or None, status[nbatch])."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        flag = int(flag_grad)
        obj = np.empty(nb)
        grad = np.empty((nb, self.H)) if flag & 1 else None
        status = np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_loo_grad(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), flag,
                                           _ptr(obj, C.c_double), _ptr(grad, C.c_double), _ptr(status, C.c_int32)))
        return obj, grad, status

    def lgo_grad(self, slots, theta, groups, flag_grad=True):
        """medgp_lgo_grad: the negative leave-group-out log pseudo-likelihood J = - sum_g lpd_g (plus the prior term, as nlml_grad)
        and its gradient in theta -- the score Context.loo(groups=...) reports, as a training objective.  groups as Context.loo
        takes them: a list of one int array of group ids per patient (-1: never held out; medgp_amd.crossval builds the usual
        partitions), "covariate", or None (classic LOO: Context.loo_grad's bits).
        Returns (obj[nbatch], grad[nbatch, H] or None, status[nbatch], [group_status[G] per patient])."""
        slots, theta, ns, gs, ng = self._loo_args(slots, theta, groups)
        nb = slots.shape[0]
        flag = int(flag_grad)
        Gs = np.array(ns if gs is None else ng, dtype=np.int64)
        goff = np.zeros(nb + 1, dtype=np.int64)
        goff[1:] = np.cumsum(Gs)
        NO, NG = int(sum(ns)), int(goff[-1])
        grp = None if gs is None else np.ascontiguousarray(np.concatenate(gs) if NO else np.zeros(1), dtype=np.int32)
        obj = np.empty(nb)
        grad = np.empty((nb, self.H)) if flag & 1 else None
        status = np.empty(nb, dtype=np.int32)
        gst = np.empty(max(NG, 1), dtype=np.int32)
        self._chk(self._lib.medgp_lgo_grad(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), _ptr(grp, C.c_int32),
                                           _ptr(ng, C.c_int32), flag, _ptr(obj, C.c_double), _ptr(grad, C.c_double),
                                           _ptr(status, C.c_int32), _ptr(gst, C.c_int32)))
        return obj, grad, status, [gst[int(goff[b]):int(goff[b + 1])].copy() for b in range(nb)]

    def fisher_vec(self, slots, theta, vecs):
        """medgp_fisher_vec: products of the Fisher information F(theta_b) = 1/2 tr(P dK_h P dK_k) of the marginal likelihood with
        directions in theta space.  slots [nbatch], theta [nbatch, H], vecs [nbatch, nvec, H] or [nbatch, H] (one direction each).
        No prior, no dependence on y.  Returns (fvec of the shape of vecs, status[nbatch]); a failed patient's rows are NaN."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        v = np.ascontiguousarray(vecs, dtype=np.float64)
        if v.ndim not in (2, 3) or v.shape[0] != nb or v.shape[-1] != self.H:
            raise ValueError(f"vecs of shape {v.shape} for {nb} patients of {self.H} hypers")
        nvec = 1 if v.ndim == 2 else v.shape[1]
        fvec = np.empty(v.shape)
        status = np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_fisher_vec(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), int(nvec),
                                             _ptr(v, C.c_double), _ptr(fvec, C.c_double), _ptr(status, C.c_int32)))
        return fvec, status

    def hess_vec(self, slots, theta, vecs, want_grad=False):
        """medgp_hess_vec: products of the exact Hessian of L = 1/2 y^T K^-1 y + 1/2 log det K (the nlml without the prior stage) with
        directions in theta space.  slots [nbatch], theta [nbatch, H], vecs [nbatch, nvec, H] or [nbatch, H] (one direction each).
        Returns (hvec of the shape of vecs, status[nbatch]), or with want_grad (hvec, grad[nbatch, H], status): grad is the gradient
        of L.  A failed patient's rows are NaN."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        v = np.ascontiguousarray(vecs, dtype=np.float64)
        if v.ndim not in (2, 3) or v.shape[0] != nb or v.shape[-1] != self.H:
            raise ValueError(f"vecs of shape {v.shape} for {nb} patients of {self.H} hypers")
        nvec = 1 if v.ndim == 2 else v.shape[1]
        hvec = np.empty(v.shape)
        grad = np.empty((nb, self.H)) if want_grad else None
        status = np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_hess_vec(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), int(nvec),
                                           _ptr(v, C.c_double), _ptr(hvec, C.c_double), _ptr(grad, C.c_double) if want_grad else None,
                                           _ptr(status, C.c_int32)))
        return (hvec, grad, status) if want_grad else (hvec, status)

    def posterior_jvp(self, slots, theta, meta2_list, t2_list, vecs, want_posterior=True):
        """medgp_posterior_jvp_batch: the directional derivatives of the posterior mean and variance at every test point along
        directions in theta space, from one factorisation per patient.  slots, theta, meta2_list, t2_list as posterior(); vecs
        [nbatch, nvec, H] or [nbatch, H] (one direction each), as fisher_vec takes it.
        Returns ([(mean[m], var[m], dmean[m, nvec], dvar[m, nvec]) per patient], status); mean and var are None without
        want_posterior.  A failed patient's rows are NaN."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        v = np.ascontiguousarray(vecs, dtype=np.float64)
        if v.ndim not in (2, 3) or v.shape[0] != p.nb or v.shape[-1] != self.H:
            raise ValueError(f"vecs of shape {v.shape} for {p.nb} patients of {self.H} hypers")
        nvec = 1 if v.ndim == 2 else v.shape[1]
        mean, var = ((np.empty(p.Mz, dtype=np.float32) if want_posterior else None) for _ in range(2))
        dmean, dvar = (np.empty((p.Mz, nvec)) for _ in range(2))
        self._chk(self._lib.medgp_posterior_jvp_batch(*p.head, *p.pts, int(nvec), _ptr(v, C.c_double), _ptr(mean, C.c_float),
                                                      _ptr(var, C.c_float), _ptr(dmean, C.c_double), _ptr(dvar, C.c_double),
                                                      _ptr(p.st, C.c_int32)))
        return list(_split(p.offsets, mean, var, dmean, dvar)), p.st

    PLOSS = {"custom": 0, "nlpd": 1, "sqerr": 2, "crps": 3}

    def posterior_vjp(self, slots, theta, meta2_list, t2_list, cot_mean=None, cot_var=None, loss=None, y2_list=None, wt_list=None,
                      want_posterior=True, fp64_posterior=False):
        """medgp_posterior_vjp_batch: the gradient in theta of a loss of the predictions, from one factorisation per patient.
        slots, theta, meta2_list, t2_list as posterior().  Either
          loss=None: cot_mean, cot_var are lists (one array per patient) of the cotangents of the patient's points, each [m] or
            [m, ncot] (the same ncot for all); returns ([(mean[m], var[m], grad[ncot, H]) per patient], status);
          loss="nlpd" | "sqerr" | "crps": y2_list (one array [m] per patient) and optionally wt_list; returns
            ([(mean[m], var[m], grad[H], loss) per patient], status).
        mean and var are None without want_posterior; with fp64_posterior they are the float64 values the device formed its
        cotangents from (medgp_posterior_vjp_moments) instead of the float outputs.  A failed patient's rows are NaN."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        nb = p.nb
        if loss is None:
            if cot_mean is None or cot_var is None or y2_list is not None or wt_list is not None:
                raise ValueError("custom cotangents: cot_mean and cot_var are required, y2_list / wt_list are not taken")
            # ncot: the columns of the first patient that has points ([m] arrays: one set)
            ncot = next((max(np.size(x) // int(m), 1) for x, m in zip(cot_mean, p.cnt) if m), 1)
            cm = self._per_point(p, cot_mean, np.float64, "cot_mean", ncot)
            cv = self._per_point(p, cot_var, np.float64, "cot_var", ncot)
            kind, y2, wt, lossv = 0, None, None, None
        else:
            if loss not in self.PLOSS or loss == "custom":
                raise ValueError(f"loss {loss!r}: one of 'nlpd', 'sqerr', 'crps', or None for custom cotangents")
            if y2_list is None or cot_mean is not None or cot_var is not None:
                raise ValueError("a built-in loss takes y2_list and no cotangents")
            kind, ncot, cm, cv = self.PLOSS[loss], 1, None, None
            y2 = self._per_point(p, y2_list, np.float64, "y2_list")
            wt = self._per_point(p, wt_list, np.float64, "wt_list")
            lossv = np.empty(nb)
        mean, var = ((np.empty(p.Mz, dtype=np.float32) if want_posterior else None) for _ in range(2))
        grad = np.empty((nb, ncot, self.H))
        self._chk(self._lib.medgp_posterior_vjp_batch(*p.head, *p.pts, kind, _ptr(y2, C.c_double), _ptr(wt, C.c_double), int(ncot),
                                                      _ptr(cm, C.c_double), _ptr(cv, C.c_double), _ptr(mean, C.c_float), _ptr(var, C.c_float),
                                                      _ptr(lossv, C.c_double), _ptr(grad, C.c_double), _ptr(p.st, C.c_int32)))
        if want_posterior and fp64_posterior:
            mean, var = np.empty(p.Mz), np.empty(p.Mz)
            self._chk(self._lib.medgp_posterior_vjp_moments(self._h, p.M, _ptr(mean, C.c_double), _ptr(var, C.c_double)))
        tails = [(grad[b].copy(),) if loss is None else (grad[b, 0].copy(), float(lossv[b])) for b in range(nb)]
        return [mv + t for mv, t in zip(_split(p.offsets, mean, var), tails)], p.st

    def _mean_args(self, nb, b0, lam, fixed, ncol=None):
        """(mode, b0 [nb, D], lam [nb, D] or None) of the baseline calls; a vector [D] serves every patient (ncol: the basis calls' p)"""
        D = ncol if ncol is not None else (self.D if self.kernel_index == KERNEL_LMC_SM else 1)

        def rows(a, what):
            a = np.asarray(a, dtype=np.float64)
            if a.size == D:
                a = np.broadcast_to(a.reshape(1, D), (nb, D))
            if a.size != nb * D:
                raise ValueError(f"{what} has {a.size} values, expected {D} or {nb} x {D}")
            return np.ascontiguousarray(a.reshape(nb, D))
        if fixed:
            if lam is not None:
                raise ValueError("fixed=True takes no lam (the mean is b0 itself)")
            return MEAN_FIXED, rows(b0, "b0"), None
        if lam is None:
            raise ValueError("lam is required unless fixed=True (medgp_amd.baseline.standard_prior / flat build it)")
        return MEAN_MARGINAL, rows(b0, "b0"), rows(lam, "lam")

    def mean_nlml_grad(self, slots, theta, b0, lam=None, fixed=False, flag_grad=True):
        """medgp_mean_nlml_grad: the nlml with a constant baseline per covariate -- fixed=True: the mean is b0 (the reference's
        c_meanfunc_constMO); else beta_d ~ N(b0_d, 1 / lam_d) is integrated out (lam_d = 0: flat).  b0, lam: [D] for every patient or
        [nbatch, D].  Returns dict(nlml [nbatch], grad [nbatch, H] or None, dmean [nbatch, D] = d nlml / d b0, beta [nbatch, D],
        beta_cov [nbatch, D, D], status [nbatch]); a failed or improper patient's rows are NaN."""
        return self._fe_nlml_grad(self._lib.medgp_mean_nlml_grad, "dmean", False, slots, theta, b0, lam, fixed, flag_grad)

    def _fe_nlml_grad(self, fn, dkey, basis, slots, theta, b0, lam, fixed, flag_grad):
        """mean_nlml_grad and basis_nlml_grad: fn the C entry point, dkey the result's key of d nlml / d b0; basis: the column count
        is the p of b0 and lam, not D"""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        mode, b0, lam = self._mean_args(nb, b0, lam, fixed, self._basis_cols(b0, lam, nb) if basis else None)
        D = b0.shape[1]
        nlml, grad = np.empty(nb), (np.empty((nb, self.H)) if flag_grad else None)
        db0, beta, cov = np.empty((nb, D)), np.empty((nb, D)), np.empty((nb, D, D))
        st = np.empty(nb, dtype=np.int32)
        self._chk(fn(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), mode, _ptr(b0, C.c_double), _ptr(lam, C.c_double),
                     int(bool(flag_grad)), _ptr(nlml, C.c_double), _ptr(grad, C.c_double), _ptr(db0, C.c_double), _ptr(beta, C.c_double),
                     _ptr(cov, C.c_double), _ptr(st, C.c_int32)))
        return {"nlml": nlml, "grad": grad, dkey: db0, "beta": beta, "beta_cov": cov, "status": st}

    def mean_posterior(self, slots, theta, meta2_list, t2_list, b0, lam=None, fixed=False):
        """medgp_mean_posterior_batch: the posterior at test points under the baseline model of mean_nlml_grad, float64.
        slots, theta, meta2_list, t2_list as posterior().  Returns ([(mean[m], var[m]) per patient], beta [nbatch, D], status)."""
        return self._fe_posterior(self._lib.medgp_mean_posterior_batch, False, slots, theta, meta2_list, t2_list, None, b0, lam, fixed)

    def _fe_posterior(self, fn, basis, slots, theta, meta2_list, t2_list, h2_list, b0, lam, fixed):
        """mean_posterior and basis_posterior: fn the C entry point; basis: the column count is the p of b0 and lam, not D, and the
        points' rows h2 ([M, p], from h2_list) go in behind t2"""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        mode, b0, lam = self._mean_args(p.nb, b0, lam, fixed, self._basis_cols(b0, lam, p.nb) if basis else None)
        h2 = [self._per_point(p, list(h2_list), np.float64, "basis", b0.shape[1])] if basis else []
        mean, var = np.empty(p.Mz), np.empty(p.Mz)
        beta = np.empty(b0.shape)
        self._chk(fn(*p.head, mode, _ptr(b0, C.c_double), _ptr(lam, C.c_double), *p.pts, *[_ptr(h, C.c_double) for h in h2],
                     _ptr(mean, C.c_double), _ptr(var, C.c_double), _ptr(beta, C.c_double), _ptr(p.st, C.c_int32)))
        return list(_split(p.offsets, mean, var)), beta, p.st

    def set_basis(self, slots, H_list):
        """medgp_set_basis: a resident basis per slot.  H_list: one [n, p] array per slot, rows in the order the patient was uploaded
        (medgp_amd.basis.Design.design builds it), the same p for all; one packed transfer, no device wait.  H_list=None removes the
        bases of the slots.  A later set_patient[s] on a slot drops its basis."""
        slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        if H_list is None:
            self._chk(self._lib.medgp_set_basis(self._h, slots.shape[0], _ptr(slots, C.c_int32), 0, None, None))
            return
        if len(H_list) != slots.shape[0]:
            raise ValueError(f"{len(H_list)} bases for {slots.shape[0]} slots")
        Hs = [np.asarray(h, dtype=np.float64) for h in H_list]
        Hs = [h.reshape(-1, 1) if h.ndim == 1 else h for h in Hs]
        p = Hs[0].shape[1]
        if any(h.ndim != 2 or h.shape[1] != p for h in Hs):
            raise ValueError("every basis of one set_basis call has the same number of columns")
        offsets = np.zeros(len(Hs) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([h.shape[0] for h in Hs])
        hm = np.ascontiguousarray(np.concatenate(Hs, axis=0) if offsets[-1] else np.zeros((1, max(p, 1))))
        self._chk(self._lib.medgp_set_basis(self._h, slots.shape[0], _ptr(slots, C.c_int32), int(p), offsets.ctypes.data_as(C.POINTER(C.c_int64)),
                                            _ptr(hm, C.c_double)))

    @staticmethod
    def _basis_cols(b0, lam, nb):
        """p of a basis call from its b0 ([p] or [nbatch, p]; lam decides where b0.size == nbatch * p is ambiguous)"""
        a = np.asarray(b0, dtype=np.float64)
        if a.ndim == 2:
            return a.shape[1]
        la = None if lam is None else np.asarray(lam, dtype=np.float64)
        return la.shape[1] if la is not None and la.ndim == 2 else a.size

    def basis_nlml_grad(self, slots, theta, b0, lam=None, fixed=False, flag_grad=True):
        """medgp_basis_nlml_grad: mean_nlml_grad with H from the slots' resident bases (set_basis) -- fixed=True: beta = b0; else
        beta_c ~ N(b0_c, 1 / lam_c) is integrated out (lam_c = 0: flat).  b0, lam: [p] for every patient or [nbatch, p].  Returns
        dict(nlml [nbatch], grad [nbatch, H] or None, dbeta [nbatch, p] = d nlml / d b0, beta [nbatch, p], beta_cov [nbatch, p, p],
        status [nbatch]); a failed patient's rows (a singular A among them) are NaN."""
        return self._fe_nlml_grad(self._lib.medgp_basis_nlml_grad, "dbeta", True, slots, theta, b0, lam, fixed, flag_grad)

    def basis_posterior(self, slots, theta, meta2_list, t2_list, h2_list, b0, lam=None, fixed=False):
        """medgp_basis_posterior_batch: the posterior at test points under the model of basis_nlml_grad, float64.  slots, theta,
        meta2_list, t2_list as posterior(); h2_list: one [m, p] array of basis rows per patient (the recipe of the observations'
        basis at the test points: medgp_amd.basis.Design.design(meta2, t2)).  Returns ([(mean[m], var[m]) per patient],
        beta [nbatch, p], status)."""
        return self._fe_posterior(self._lib.medgp_basis_posterior_batch, True, slots, theta, meta2_list, t2_list, h2_list, b0, lam, fixed)

    def _warp_args(self, nb, psi, kind):
        """psi as [nbatch, D, 3] (one [D, 3] block serves every patient), kind as int32 [D] or None = all SAS"""
        D = self.D if self.kernel_index == KERNEL_LMC_SM else 1
        a = np.asarray(psi, dtype=np.float64)
        if a.size == D * 3:
            a = np.broadcast_to(a.reshape(1, D, 3), (nb, D, 3))
        elif a.size != nb * D * 3:
            raise ValueError(f"psi has {a.size} values, expected {D} x 3 or {nb} x {D} x 3")
        if kind is not None:
            kind = np.ascontiguousarray(kind, dtype=np.int32).ravel()
            if kind.shape[0] != D:
                raise ValueError(f"kind has {kind.shape[0]} entries, expected {D}")
        return D, np.ascontiguousarray(a.reshape(nb, D, 3)), kind

    def warp_nlml_grad(self, slots, theta, psi, kind=None, flag_grad=True):
        """medgp_warp_nlml_grad: the nlml of the warped GP z = g_d(y) with the sinh-arcsinh map per covariate (medgp_amd.warp), and
        its gradients in theta and psi.  psi: [D, 3] for every patient or [nbatch, D, 3], rows (a, eps, lambda); kind: [D] of
        WARP_NONE / WARP_SAS, None = all SAS.  Returns dict(nlml [nbatch], grad [nbatch, H] or None, dpsi [nbatch, D, 3],
        logjac [nbatch], status [nbatch]); a failed patient's rows (a warped observation that is not finite among them) are NaN."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        D, psi, kind = self._warp_args(nb, psi, kind)
        nlml, grad = np.empty(nb), (np.empty((nb, self.H)) if flag_grad else None)
        dpsi, logjac, st = np.empty((nb, D, 3)), np.empty(nb), np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_warp_nlml_grad(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), _ptr(kind, C.c_int32),
                                                 _ptr(psi, C.c_double), int(bool(flag_grad)), _ptr(nlml, C.c_double), _ptr(grad, C.c_double),
                                                 _ptr(dpsi, C.c_double), _ptr(logjac, C.c_double), _ptr(st, C.c_int32)))
        return {"nlml": nlml, "grad": grad, "dpsi": dpsi, "logjac": logjac, "status": st}

    def warp_posterior(self, slots, theta, psi, meta2_list, t2_list, y2_list=None, probs=(0.025, 0.5, 0.975), kind=None, zq=None):
        """medgp_warp_posterior_batch: the warped posterior at test points, float64.  slots, theta, meta2_list, t2_list as
        posterior(); psi, kind as warp_nlml_grad; y2_list: the observed values at the points (one array per patient) for lpd;
        probs: the probabilities of the quantiles (they become standard-normal deviates on the host); zq: the deviates themselves --
        when zq is given, probs is ignored.  Returns
        ([dict(zmean [m], zvar [m], quant [m, len(probs)], lpd [m] or None) per patient], status)."""
        from statistics import NormalDist
        p = self._point_args(slots, theta, meta2_list, t2_list)
        D, psi, kind = self._warp_args(p.nb, psi, kind)
        if zq is None:
            probs = [float(p) for p in probs]
            if any(not 0.0 < p < 1.0 for p in probs):
                raise ValueError("probs lie strictly between 0 and 1")
            nd = NormalDist()
            zq = [0.0 if p == 0.5 else nd.inv_cdf(p) for p in probs]
        zq = np.ascontiguousarray(zq, dtype=np.float64).ravel()
        nq = zq.shape[0]
        y2 = self._per_point(p, y2_list, np.float32, "y2")
        zmean, zvar = np.empty(p.Mz), np.empty(p.Mz)
        quant = np.empty((p.Mz, nq)) if nq else None
        lpd = np.empty(p.Mz) if y2 is not None else None
        self._chk(self._lib.medgp_warp_posterior_batch(*p.head, _ptr(kind, C.c_int32), _ptr(psi, C.c_double), *p.pts, _ptr(y2, C.c_float), nq,
                                                       _ptr(zq, C.c_double) if nq else None, _ptr(zmean, C.c_double), _ptr(zvar, C.c_double),
                                                       _ptr(quant, C.c_double), _ptr(lpd, C.c_double), _ptr(p.st, C.c_int32)))
        return [dict(zmean=a, zvar=v, quant=q, lpd=l) for a, v, q, l in _split(p.offsets, zmean, zvar, quant, lpd)], p.st

    # ---- per-observation noise scales and Student-t robust training (include/medgp_hip.h; helpers: medgp_amd.robust) ----
    def _rows_of(self, slots):
        """(n per entry, CSR offsets [nbatch + 1]) of the observations of the entries' patients"""
        ns = np.array([self._slot_n[int(s)] for s in slots], dtype=np.int64)
        off = np.zeros(ns.shape[0] + 1, dtype=np.int64)
        off[1:] = np.cumsum(ns)
        return ns, off

    def _pack_rows(self, slots, rows, what):
        """one array per entry, one value per observation in the order the patient was uploaded -> one packed float64 array"""
        ns, off = self._rows_of(slots)
        if len(rows) != ns.shape[0]:
            raise ValueError(f"{len(rows)} {what} arrays for {ns.shape[0]} patients")
        arrs = [np.asarray(r, dtype=np.float64).ravel() for r in rows]
        for b, (a, n) in enumerate(zip(arrs, ns)):
            if a.shape[0] != n:
                raise ValueError(f"patient {b}: {a.shape[0]} {what} values for {int(n)} observations")
        return off, np.ascontiguousarray(np.concatenate(arrs) if off[-1] else np.ones(1))

    def set_noise_scale(self, slots, scales):
        """medgp_set_noise_scale: resident per-observation noise scales s_i > 0 (the noise variance of row i is sigma^2_{m_i} s_i) for
        hetero_nlml_grad and hetero_posterior; every other call ignores them.  scales: one array per slot, one value per observation
        in the order the patient was uploaded (medgp_amd.robust.from_replicates / from_sd / flagged build them); None drops the
        slots' tables.  A later set_patient[s] on a slot drops its table."""
        slots = np.ascontiguousarray(slots, dtype=np.int32).ravel()
        if scales is None:
            self._chk(self._lib.medgp_set_noise_scale(self._h, slots.shape[0], _ptr(slots, C.c_int32), None, None))
            return
        off, sc = self._pack_rows(slots, scales, "scale")
        self._chk(self._lib.medgp_set_noise_scale(self._h, slots.shape[0], _ptr(slots, C.c_int32), _ptr(off, C.c_int64), _ptr(sc, C.c_double)))

    def hetero_nlml_grad(self, slots, theta, flag_grad=True, rows=True):
        """medgp_hetero_nlml_grad: nlml and gradient under the slots' resident noise scales, and (rows=True) per training row
        resid = y - E f and fvar = var f.  Returns dict(nlml [nbatch], grad [nbatch, H] or None, resid, fvar: lists of one array [n]
        per patient or None, status [nbatch]); a failed patient's rows are NaN."""
        slots, theta = self._batch_args(slots, theta, check=True)
        nb = slots.shape[0]
        _, off = self._rows_of(slots)
        nlml, grad, st = np.empty(nb), (np.empty((nb, self.H)) if flag_grad else None), np.empty(nb, dtype=np.int32)
        resid = np.empty(max(int(off[-1]), 1)) if rows else None
        fvar = np.empty(max(int(off[-1]), 1)) if rows else None
        self._chk(self._lib.medgp_hetero_nlml_grad(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), int(bool(flag_grad)),
                                                   _ptr(nlml, C.c_double), _ptr(grad, C.c_double), _ptr(resid, C.c_double), _ptr(fvar, C.c_double),
                                                   _ptr(st, C.c_int32)))
        sp = list(_split(off, resid, fvar))
        return {"nlml": nlml, "grad": grad, "resid": [x[0] for x in sp] if rows else None, "fvar": [x[1] for x in sp] if rows else None, "status": st}

    def hetero_posterior(self, slots, theta, meta2_list, t2_list, s2_list=None):
        """medgp_hetero_posterior_batch: the posterior at test points under the slots' resident noise scales, float64.  slots, theta,
        meta2_list, t2_list as posterior(); s2_list: the noise scale of every point (one array per patient; None: 1, a 0: the latent
        f).  Returns ([(mean[m], var[m]) per patient], status)."""
        p = self._point_args(slots, theta, meta2_list, t2_list)
        s2 = self._per_point(p, s2_list, np.float64, "s2")
        mean, var = np.empty(p.Mz), np.empty(p.Mz)
        self._chk(self._lib.medgp_hetero_posterior_batch(*p.head, *p.pts, _ptr(s2, C.c_double), _ptr(mean, C.c_double), _ptr(var, C.c_double),
                                                         _ptr(p.st, C.c_int32)))
        return list(_split(p.offsets, mean, var)), p.st

    def robust_nlml_grad(self, slots, theta, nu, sweeps=3, scale0=None, flag_grad=True, rows=True):
        """medgp_robust_nlml_grad: Student-t noise by variational reweighting -- `sweeps` E-steps from scale0 (one array per patient
        in the order it was uploaded; None: ones), then the bound J, its gradient and the row statistics at the last scales.
        nu: the degrees of freedom, a scalar, [D] for every patient or [nbatch, D] (SE / SM: D = 1).  Returns dict(obj [nbatch],
        grad [nbatch, H] or None, scale, resid, fvar: lists of one array [n] per patient (resid, fvar None without rows),
        delta [nbatch], status [nbatch]); a failed patient's rows are NaN."""
        slots, theta = self._batch_args(slots, theta, check=True)
        nb = slots.shape[0]
        D = self.D if self.kernel_index == KERNEL_LMC_SM else 1
        nu = np.asarray(nu, dtype=np.float64)
        if nu.size not in (1, D, nb * D):
            raise ValueError(f"nu has {nu.size} values, expected 1, {D} or {nb} x {D}")
        nu = np.ascontiguousarray(nu.reshape(nb, D) if nu.size == nb * D else np.broadcast_to(nu.reshape(1, -1), (nb, D)))
        _, off = self._rows_of(slots)
        s0 = None if scale0 is None else self._pack_rows(slots, scale0, "scale0")[1]
        nrow = max(int(off[-1]), 1)
        obj, grad, st = np.empty(nb), (np.empty((nb, self.H)) if flag_grad else None), np.empty(nb, dtype=np.int32)
        scale, delta = np.empty(nrow), np.empty(nb)
        resid, fvar = (np.empty(nrow), np.empty(nrow)) if rows else (None, None)
        self._chk(self._lib.medgp_robust_nlml_grad(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), _ptr(nu, C.c_double), int(sweeps),
                                                   _ptr(s0, C.c_double), int(bool(flag_grad)), _ptr(obj, C.c_double), _ptr(grad, C.c_double),
                                                   _ptr(scale, C.c_double), _ptr(resid, C.c_double), _ptr(fvar, C.c_double), _ptr(delta, C.c_double),
                                                   _ptr(st, C.c_int32)))
        sp = list(_split(off, scale, resid, fvar))
        return {"obj": obj, "grad": grad, "scale": [x[0] for x in sp], "resid": [x[1] for x in sp] if rows else None,
                "fvar": [x[2] for x in sp] if rows else None, "delta": delta, "status": st}

    def forecast_grad(self, slots, theta, prefixes=None, flag_grad=1):
        """medgp_forecast_grad: the negative forecast score J = - sum_i lpd_i (plus the prior term, as nlml_grad) and its gradient in
        theta.  prefixes: one int array per patient, in the order the patient was uploaded: prefixes[b][i] = the number of leading
        observations observation i is predicted from (0 <= p <= i), or -1 = not scored (medgp_amd.forecast.training_prefix builds it
        from times and a horizon); None = every observation from all before it, the chain rule of the likelihood.
        Returns (obj[nbatch], grad[nbatch, H] or None, status[nbatch])."""
        slots, theta = self._batch_args(slots, theta)
        nb = slots.shape[0]
        flag = int(flag_grad)
        offsets = prefix = None
        if prefixes is not None:
            if len(prefixes) != nb:
                raise ValueError(f"{len(prefixes)} prefix arrays for {nb} patients")
            pl = [np.asarray(p, dtype=np.int32).ravel() for p in prefixes]
            offsets = np.zeros(nb + 1, np.int64)
            offsets[1:] = np.cumsum([p.shape[0] for p in pl])
            prefix = np.ascontiguousarray(np.concatenate(pl) if pl else np.zeros(0, np.int32), dtype=np.int32)
            if prefix.shape[0] == 0:
                prefix = np.zeros(1, np.int32)   # (never read: every range is empty)
        obj = np.empty(nb)
        grad = np.empty((nb, self.H)) if flag & 1 else None
        status = np.empty(nb, dtype=np.int32)
        self._chk(self._lib.medgp_forecast_grad(self._h, nb, _ptr(slots, C.c_int32), _ptr(theta, C.c_double), _ptr(offsets, C.c_int64),
                                                _ptr(prefix, C.c_int32), flag, _ptr(obj, C.c_double), _ptr(grad, C.c_double),
                                                _ptr(status, C.c_int32)))
        return obj, grad, status

    def synchronize(self):
        self._chk(self._lib.medgp_synchronize(self._h))

    # measurement hooks
    def profile_enable(self, on=True, only=None):
        """on: bracket every launch with HIP events; only='k_cholinv': just the launches of that kernel."""
        mode = int(bool(on))
        if on and only is not None:
            names = [self._lib.medgp_profile_kernel_name_ext3(k).decode() for k in range(self._lib.medgp_profile_num_kernels_ext3())]
            mode = 2 + names.index(only)
        self._chk(self._lib.medgp_profile_enable(self._h, mode))
        self._profile_only = mode - 2 if mode >= 2 else None

    def profile_reset(self):
        self._chk(self._lib.medgp_profile_reset(self._h))

    def profile_read(self, all_entries=False):
        """{kernel name: (milliseconds, launches)} of the entries [0, medgp_profile_num_kernels_ext()), the table callers compare as a
        whole; all_entries=True: also the entries added since (the warp calls' four kernels), up to medgp_profile_num_kernels_ext2().
        A kernel beyond the table that profile_enable(only=...) last named is returned as well: what was asked for is never left out
        (the heteroscedastic calls' five kernels, ids up to medgp_profile_num_kernels_ext3(), are reached that way)."""
        out = {}
        ids = list(range(self._lib.medgp_profile_num_kernels_ext2() if all_entries else self._lib.medgp_profile_num_kernels_ext()))
        only = getattr(self, "_profile_only", None)
        if only is not None and only not in ids:
            ids.append(only)
        for k in ids:
            ms, cnt = C.c_double(), C.c_int64()
            self._chk(self._lib.medgp_profile_read(self._h, k, C.byref(ms), C.byref(cnt)))
            out[self._lib.medgp_profile_kernel_name_ext3(k).decode()] = (ms.value, cnt.value)
        return out
