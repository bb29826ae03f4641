// kernels_hetero.h -- per-observation noise scales and Student-t robust training (medgp_set_noise_scale, medgp_hetero_nlml_grad,
// medgp_hetero_posterior_batch, medgp_robust_nlml_grad).  Row i of covariate d = m_i carries a scale s_i > 0; with r jitter rounds the
// factored noise is N_i = (1 + r) sigma^2_d s_i and K_s = K + diag(N), P = K_s^-1, alpha = P y:
//   nlml = 1/2 y^T alpha + 1/2 log|K_s| + 1/2 n log 2 pi,   d nlml / d theta_h = 1/2 tr((P - alpha alpha^T) dK_s / d theta_h),
//   the noise hyper of covariate d: sigma^2_d sum_{m_i = d} s_i W_ii  (the existing noise line with s_i W_ii in the place of W_ii),
//   resid_i = y_i - E f_i = N_i alpha_i,   fvar_i = var f_i = N_i - N_i^2 P_ii,   P_ii = wdiag_i + alpha_i^2.
// The scales enter where the noise vector enters: k_assemble_t<QT, 0, true> and reassemble_wg read MedgpDev::nscale when it is set
// (null in every other call); the factorisation, k_wgrad, k_slabsum and k_epilogue run unchanged.  k_assemble_v0 does not read it: these
// calls refuse Q > 16 and always take the templated kernels.
// Student-t noise as a Gaussian scale mixture (robust_tables.h), by variational reweighting: one E-step from a factorisation at s is
//   e_i = (resid_i^2 + fvar_i) / sigma^2_{m_i},   s_i <- (nu_d + e_i) / (nu_d + 1),
// and the objective is J = nlml(theta; s) + sum_i c_d (log s_i + 1 / s_i) + sum_d n_d C(nu_d).  The definition is tests/hetero_truth.py.
//
//   k_het_load   the slot-resident scales (grouped order) into the entry table; ones where a slot has none and for the padding rows
//   k_het_rows   behind the unchanged k_wgrad: resid and fvar of every row, then wdiag_i *= s_i in place (k_epilogue's noise line then
//                yields the heteroscedastic gradient as it stands)
//   k_het_estep  e_i, the new s_i into the entry table, and delta = max_i |s_new - s_old| / s_new of the entry
//   k_het_obj    sum_i c_d (log s_i + 1 / s_i) + sum_d n_d C_d on top of the nlml of the factorisation -> scal[2] (k_epilogue's
//                supplied-objective mode)
//   k_het_post   behind the unchanged k_pjvp_solve (V = L^-1 K* per tile of 64 points): mean = V^T z, var = k** - V^T V + sigma^2 s2
// fp64, wave64, no atomics; every sum in a fixed order over operands of the entry alone: an entry's bits depend neither on its
// batch-mates nor on its position or the batch size (with the route pinned, as everywhere).
#pragma once
#include "kernels_posterior_jvp.h"
#include "hetero_tables.h"
#include "robust_tables.h"

// the covariate of grouped row i: the d with seg[d] <= i < seg[d + 1] (covariates without observations have empty ranges)
__device__ __forceinline__ int het_row_cov(const int *__restrict__ seg, int D, int i) {
    int lo = 0, hi = D - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the larger of two values, NaN if either is
__device__ __forceinline__ double het_max_nan(double a, double b) { return (a != a || b != b) ? __builtin_nan("") : fmax(a, b); }

// ------------------------------------------------------------------------------------------
// grid = (256-row blocks of the class's leading dimension, entries).  has: [entries of the class] 1 = the entry's slot has resident
// scales; slot_scale: [max_slots][pld] in the grouped order, or null (no slot of the context has any).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_het_load(MedgpDev L, const int *__restrict__ has, const double *__restrict__ slot_scale,
                                                  double *__restrict__ sv) {
    const int b = blockIdx.y, i = 256 * (int)blockIdx.x + (int)threadIdx.x;
    const int ld = L.ldn;
    if (i >= ld) return;
    const int slot = L.bslot[b], n = L.pn[slot];
    double s = 1.0;
    if (slot_scale && has[b] && i < n) s = slot_scale[(size_t)slot * L.pld + i];
    sv[het_vec_at(b, ld, i)] = s;
}

// ------------------------------------------------------------------------------------------
// grid = (256-row blocks of the class's leading dimension, entries).  with_w: k_wgrad has run (wdiag holds diag(P - alpha alpha^T));
// without it only resid is formed and fvar is left alone.  The status of a factored entry is its jitter rounds r; N_i is summed as the
// assembly sums it (lik added 1 + r times).  Rows n .. ld of resid and fvar are zero.  A failed entry writes nothing.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_het_rows(MedgpDev L, const double *__restrict__ sv, int with_w, double *__restrict__ resid,
                                                  double *__restrict__ fvar) {
    const int b = blockIdx.y, i = 256 * (int)blockIdx.x + (int)threadIdx.x;
    const int ld = L.ldn, st = L.status[b];
    if (i >= ld || st < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], D = L.D;
    const size_t at = het_vec_at(b, ld, i);
    double r = 0.0, f = 0.0;
    if (i < n) {
        const int d = het_row_cov(L.pseg + (size_t)slot * (D + 1), D, i);
        const double s = sv[at], lik = L.hyp[(size_t)b * L.hyp_stride + d] * s;
        double N = lik;
        for (int k = 0; k < st; k++) N += lik;
        const double a = L.alpha[at];
        r = N * a;
        if (with_w) {
            const double w = L.wdiag[at];
            f = N - (N * N) * (w + a * a);
            L.wdiag[at] = w * s;
        }
    }
    resid[at] = r;
    if (with_w) fvar[at] = f;
}

// ------------------------------------------------------------------------------------------
// grid = the class's entries, 256 threads.  tab: robust_tables.h, the caller's entry order.  sv is read and written (no __restrict__).
// The maximum is exact in any order, and a new scale that is not finite makes delta NaN (het_max_nan: fmax alone would drop it).  A
// failed entry gets NaN scales (every later factorisation of the call then fails for it: the entry ends with status -1) and delta NaN.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_het_estep(MedgpDev L, const double *__restrict__ tab, double *sv, const double *__restrict__ resid,
                                                   const double *__restrict__ fvar, double *__restrict__ delta) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D;
    const int pos = L.bpos ? L.bpos[b] : b;
    if (L.status[b] < 0) {
        const double nan = __builtin_nan("");
        for (int i = tid; i < n; i += 256) sv[het_vec_at(b, ld, i)] = nan;
        if (tid == 0) delta[pos] = nan;
        return;
    }
    const int *seg = L.pseg + (size_t)slot * (D + 1);
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    double dmax = 0.0;
    for (int i = tid; i < n; i += 256) {
        const int d = het_row_cov(seg, D, i);
        const size_t at = het_vec_at(b, ld, i);
        const double nu = tab[robust_tab_at(pos, D, d, ROBUST_TAB_NU)];
        const double r = resid[at], e = (r * r + fvar[at]) / hyp[d];
        const double so = sv[at], sn = (nu + e) / (nu + 1.0);
        sv[at] = sn;
        dmax = het_max_nan(dmax, isfinite(sn) ? fabs(sn - so) / sn : __builtin_nan(""));
    }
    red[tid] = dmax;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] = het_max_nan(red[tid], red[tid + off]);
        __syncthreads();
    }
    if (tid == 0) delta[pos] = red[0];
}

// ------------------------------------------------------------------------------------------
// grid = the class's entries, 256 threads.  A wave per covariate (lane l the rows seg[d] + l, + 64, ... in order, then a fixed
// butterfly, as k_epilogue's par_sig); the covariates are added in order by one thread.  scal[2] = the nlml of the factorisation as
// k_epilogue forms it, plus the sum.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_het_obj(MedgpDev L, const double *__restrict__ tab, const double *__restrict__ sv) {
    __shared__ double s_cov[MEDGP_MAX_D];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, c = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D;
    const int pos = L.bpos ? L.bpos[b] : b;
    const int *seg = L.pseg + (size_t)slot * (D + 1);
    for (int d = c; d < D; d += 4) {
        const double cd = tab[robust_tab_at(pos, D, d, ROBUST_TAB_C)];
        double acc = 0.0;
        for (int i = seg[d] + lane; i < seg[d + 1]; i += 64) {
            const double s = sv[het_vec_at(b, ld, i)];
            acc += cd * (log(s) + 1.0 / s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) s_cov[d] = acc + (double)(seg[d + 1] - seg[d]) * tab[robust_tab_at(pos, D, d, ROBUST_TAB_CONST)];
    }
    __syncthreads();
    if (tid == 0) {
        double k = 0.0;
        for (int d = 0; d < D; d++) k += s_cov[d];
        const double logdet = L.scal[b * 4 + 0], quad = L.scal[b * 4 + 1];
        L.scal[b * 4 + 2] = (quad / 2.0 + logdet + n * log(2. * L.pi) / 2.0) + k;
    }
}

// ------------------------------------------------------------------------------------------
// grid = the chunk's tiles (k_pjvp_solve of the same chunk left V behind the first panel of every tile's work rows).  Thread (point =
// tid mod 64, class = tid / 64): the two moments in four row classes per point, rows in order within a class, the classes added in a
// fixed order (k_warp_post's cut).  s2: the scale of every point's noise, or null = 1 (0: the latent f).  Outputs in the call's point
// order; the points of a failed entry get NaN.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_het_post(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                  const double *__restrict__ work, size_t work_stride, const double *__restrict__ s2,
                                                  double *__restrict__ mean, double *__restrict__ var) {
    __shared__ double part[2][4][64];
    const PostTile T = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, c = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = T.e;
    const size_t pt = (size_t)T.p0 + lane;
    if (L.status[b] < 0) {
        if (c == 0 && lane < T.cnt) {
            mean[pt] = __builtin_nan("");
            var[pt] = __builtin_nan("");
        }
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, Q = L.Q;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride, *B = hyp + hyp_off_B(L);
    const double *z = L.z + (size_t)b * ld;
    const double *Vf = work + (size_t)blockIdx.x * work_stride + (size_t)ld * 64;
    {
        double s1 = 0.0, sq = 0.0;
        if (lane < T.cnt)
            for (int i = c; i < n; i += 4) {
                const double v = Vf[(size_t)i * 64 + lane];
                s1 += v * z[i];
                sq += v * v;
            }
        part[0][c][lane] = s1;
        part[1][c][lane] = sq;
    }
    __syncthreads();
    if (tid < T.cnt) {
        const int m2 = meta2[pt];
        const double mu = ((part[0][0][tid] + part[0][1][tid]) + part[0][2][tid]) + part[0][3][tid];
        const double vv = ((part[1][0][tid] + part[1][1][tid]) + part[1][2][tid]) + part[1][3][tid];
        double kss = 0.0;
        for (int q = 0; q < Q; q++) kss += B[(size_t)q * D * D + m2 * D + m2];
        mean[pt] = mu;
        var[pt] = (kss - vv) + (s2 ? hyp[m2] * s2[pt] : hyp[m2]);
    }
}
