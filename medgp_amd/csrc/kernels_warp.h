// kernels_warp.h -- a learned monotone output warp per covariate (medgp_warp_nlml_grad, medgp_warp_posterior_batch): a warped GP
// (Snelson, Rasmussen & Ghahramani 2004) with the sinh-arcsinh family (Jones & Pewsey 2009).  Every other call is Gaussian in the
// observed value; here z = g_d(y) is, with psi_d = (a, eps, lambda), delta = exp(lambda), s = asinh(y), u = delta s - eps:
//   z = a + sinh(u),   log g' = lambda + log cosh(u) - 1/2 log(1 + y^2),   g^-1(z) = sinh((asinh(z - a) + eps) / delta)
//   dz / d(a, eps, lambda) = (1, -cosh u, delta s cosh u),   dlog g' / d(a, eps, lambda) = (0, -tanh u, 1 + delta s tanh u)
// kind[d] = MEDGP_WARP_NONE: z = y, log g' = 0, dpsi = 0.  Works behind one unchanged pipeline run that left L and U = L^-T.  With
// P = K^-1 = U U^T, w = L^-1 z = U^T z, alpha~ = P z = U w:
//   nlml = 1/2 |w|^2 + 1/2 log|K| + 1/2 n log 2 pi - sum_i log g'_i,   d nlml / d theta_h = 1/2 tr((P - alpha~ alpha~^T) dK/dtheta_h),
//   dpsi[d][k] = sum_{m_i = d} (alpha~_i dz_i/dpsi_k - dlog g'_i/dpsi_k).  The definition is tests/warp_truth.py.
//
//   k_warp_z      z_i and log g'_i of every row in the pipeline's grouped order (a row's covariate from pseg); a z_i that is not finite
//                 (sinh overflowed) gives the entry status -1
//   k_warp_solve  w = U^T z and alpha~ = U w over the upper triangle of U, one workgroup per entry; the cut is warp_tables.h's
//   k_warp_small  1/2 |w|^2, sum log g', the segmented sums dpsi over each covariate's rows (the derivative triples recomputed from y
//                 and psi), and the objective (-> scal[2], where k_epilogue's supplied-objective mode reads it)
//   k_wgrad, k_slabsum, k_epilogue (unchanged) on a view whose alpha is alpha~
//   k_warp_post   behind the unchanged k_pjvp_solve (V = L^-1 K* per tile of 64 points): zmean = V^T w, zvar = k** - V^T V + sigma^2,
//                 the quantiles g^-1(zmean + zq_k sqrt(zvar)) and lpd = log N(g(y2); zmean, zvar) + log g'(y2), all fp64
// No atomics; every sum in a fixed order over operands of the entry alone: an entry's bits depend neither on its batch-mates, nor on
// its position, the batch size or the launch chunk (with the route pinned, as everywhere); a point's neither on the other points nor
// on the tile column it lands in.
#pragma once
#include "kernels_posterior_jvp.h"
#include "warp_tables.h"

struct WarpPsi { double a, eps, delta, lam; };
__device__ __forceinline__ WarpPsi warp_psi(const double *__restrict__ psi, int pos, int D, int d) {
    WarpPsi p;
    p.a = psi[warp_in_psi(pos, D, d, 0)];
    p.eps = psi[warp_in_psi(pos, D, d, 1)];
    p.lam = psi[warp_in_psi(pos, D, d, 2)];
    p.delta = exp(p.lam);
    return p;
}
// log cosh(u) without overflow: |u| + log(1 + exp(-2 |u|)) - log 2
__device__ __forceinline__ double warp_logcosh(double u) {
    const double au = fabs(u);
    return au + log1p(exp(-2.0 * au)) - 0.693147180559945309417;
}
// z = g(y) and log g'(y)
__device__ __forceinline__ void warp_forward(const WarpPsi &p, double y, double &z, double &lj) {
    const double u = p.delta * asinh(y) - p.eps;
    z = p.a + sinh(u);
    lj = p.lam + warp_logcosh(u) - 0.5 * log1p(y * y);
}
__device__ __forceinline__ double warp_inverse(const WarpPsi &p, double z) { return sinh((asinh(z - p.a) + p.eps) / p.delta); }

// the covariate of grouped row i: the d with seg[d] <= i < seg[d + 1] (covariates without observations have empty ranges)
__device__ __forceinline__ int warp_row_cov(const int *__restrict__ seg, int D, int i) {
    int lo = 0, hi = D - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------
// grid = (256-row blocks of the class's leading dimension, entries).  kind: [D] or null (all SAS); psi: the call's, caller's order.
// Rows n .. ld of z and log g' are zero.  A non-finite z_i: status -1 (every writer stores the same word).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_warp_z(MedgpDev L, const int *__restrict__ kind, const double *__restrict__ psi,
                                                double *__restrict__ zv, double *__restrict__ ljv) {
    const int b = blockIdx.y, i = 256 * (int)blockIdx.x + (int)threadIdx.x;
    const int ld = L.ldn;
    if (i >= ld) return;
    const int slot = L.bslot[b], n = L.pn[slot], D = L.D;
    double z = 0.0, lj = 0.0;
    if (i < n && n >= 1) {
        const int d = warp_row_cov(L.pseg + (size_t)slot * (D + 1), D, i);
        const double y = L.py[(size_t)slot * L.pld + i];
        z = y;
        if (!kind || kind[d] == MEDGP_WARP_SAS) warp_forward(warp_psi(psi, L.bpos ? L.bpos[b] : b, D, d), y, z, lj);
        if (!isfinite(z)) L.status[b] = -1;
    }
    zv[warp_vec_at(b, ld, i)] = z;
    ljv[warp_vec_at(b, ld, i)] = lj;
}

// ------------------------------------------------------------------------------------------
// grid = the class's entries, WARP_SOLVE_THREADS threads.  Readers of U mask row <= column (medgp_dev.h) and column < n.
// (wv is written and read here: no __restrict__ on it)
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WARP_SOLVE_THREADS) k_warp_solve(MedgpDev L, const double *__restrict__ zv, double *wv, double *__restrict__ atv) {
    __shared__ double part[WARP_SOLVE_CLASSES][WARP_SOLVE_COLS];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, c = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const double *U = L.Linv + (size_t)b * ld * ld;
    const double *z = zv + warp_vec_at(b, ld, 0);
    double *w = wv + warp_vec_at(b, ld, 0), *at = atv + warp_vec_at(b, ld, 0);
    const int ncb = warp_solve_blocks(npad);
    for (int i = npad + tid; i < ld; i += WARP_SOLVE_THREADS) { w[i] = 0.0; at[i] = 0.0; }
    // w = U^T z: w_i = sum_{j <= i} U[j][i] z_j
    for (int cb = 0; cb < ncb; cb++) {
        const int i0 = warp_solve_col(cb, lane), j1 = warp_solve_rows(cb, n);
        double s0 = 0.0, s1 = 0.0;
        if (i0 < npad) {
            // the rows above the block's own diagonal square are full width: no mask, the loads of several rows in flight (the same
            // rows in the same order as one masked loop: 128 cb is a multiple of the class count and lies below n)
            const int jf = cb * WARP_SOLVE_COLS;
#pragma unroll 8
            for (int j = c; j < jf; j += WARP_SOLVE_CLASSES) {
                const double2 u = *reinterpret_cast<const double2 *>(U + (size_t)j * ld + i0);
                const double zj = z[j];
                s0 += u.x * zj;
                s1 += u.y * zj;
            }
            for (int j = jf + c; j < j1; j += WARP_SOLVE_CLASSES) {
                if (j <= i0 + 1) {
                    const double2 u = *reinterpret_cast<const double2 *>(U + (size_t)j * ld + i0);
                    const double zj = z[j];
                    if (j <= i0) s0 += u.x * zj;
                    s1 += u.y * zj;
                }
            }
        }
        part[c][2 * lane] = s0;
        part[c][2 * lane + 1] = s1;
        __syncthreads();
        if (tid < WARP_SOLVE_COLS) {
            const int i = cb * WARP_SOLVE_COLS + tid;
            if (i < npad) w[i] = (i < n) ? ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid] : 0.0;
        }
        __syncthreads();
    }
    // alpha~ = U w: alpha~_j = sum_{i >= j} U[j][i] w_i, a wave per row
    for (int j = c; j < npad; j += WARP_SOLVE_CLASSES) {
        double s = 0.0;
        if (j < n) {
            const double *Ur = U + (size_t)j * ld;
            for (int cb = warp_solve_first_block(j); cb < ncb; cb++) {
                const int i0 = warp_solve_col(cb, lane);
                if (i0 < npad && i0 + 1 >= j && i0 < n) {
                    const double2 u = *reinterpret_cast<const double2 *>(Ur + i0);
                    const double w0 = w[i0], w1 = w[i0 + 1];
                    if (i0 >= j) s += u.x * w0;
                    if (i0 + 1 < n) s += u.y * w1;
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        }
        if (lane == 0) at[j] = s;
    }
}

// ------------------------------------------------------------------------------------------
// grid = the class's entries.  small: the class's part of the per-entry blocks (warp_tables.h).  A covariate without observations, or of
// kind NONE: dpsi = 0 exactly.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_warp_small(MedgpDev L, const int *__restrict__ kind, const double *__restrict__ psi,
                                                    const double *__restrict__ ljv, const double *__restrict__ wv,
                                                    const double *__restrict__ atv, double *__restrict__ small) {
    __shared__ double red[2][256];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, c = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D;
    const int pos = L.bpos ? L.bpos[b] : b;
    const int *seg = L.pseg + (size_t)slot * (D + 1);
    const double *y = L.py + (size_t)slot * L.pld;
    const double *lj = ljv + warp_vec_at(b, ld, 0), *w = wv + warp_vec_at(b, ld, 0), *at = atv + warp_vec_at(b, ld, 0);
    double *sm = small + (size_t)b * warp_small_stride(D);
    // 1/2 |w|^2 and sum log g': per thread the rows tid, tid + 256, ... in order, then one fixed tree
    {
        double q = 0.0, s = 0.0;
        for (int i = tid; i < n; i += 256) {
            q += w[i] * w[i];
            s += lj[i];
        }
        red[0][tid] = q;
        red[1][tid] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) { red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off]; }
            __syncthreads();
        }
    }
    // dpsi: a wave per covariate, lane l the rows seg[d] + l, + 64, ... in order, then a fixed butterfly
    for (int d = c; d < D; d += 4) {
        double sa = 0.0, se = 0.0, sl = 0.0;
        if (!kind || kind[d] == MEDGP_WARP_SAS) {
            const WarpPsi p = warp_psi(psi, pos, D, d);
            for (int i = seg[d] + lane; i < seg[d + 1]; i += 64) {
                const double s = asinh(y[i]), u = p.delta * s - p.eps, ch = cosh(u), th = tanh(u), a = at[i];
                sa += a;
                se += th - a * ch;
                sl += a * (p.delta * s * ch) - (1.0 + p.delta * s * th);
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                sa += __shfl_xor(sa, off);
                se += __shfl_xor(se, off);
                sl += __shfl_xor(sl, off);
            }
        }
        if (lane == 0) {
            sm[warp_off_dpsi(d, 0)] = sa;
            sm[warp_off_dpsi(d, 1)] = se;
            sm[warp_off_dpsi(d, 2)] = sl;
        }
    }
    if (tid == 0) {
        const double hq = red[0][0] / 2.0, logjac = red[1][0];
        sm[warp_off_logjac()] = logjac;
        sm[warp_off_quad()] = hq;
        // (scal[0] = sum log diag L = 1/2 log|K|, as k_epilogue reads it)
        L.scal[b * 4 + 2] = ((hq + L.scal[b * 4 + 0]) + n * log(2. * L.pi) / 2.0) - logjac;
    }
}

// ------------------------------------------------------------------------------------------
// grid = the chunk's tiles (k_pjvp_solve of the same chunk left V behind the first panel of every tile's work rows).  Thread (point =
// tid mod 64, class = tid / 64): the two moments in four row classes per point, rows in order within a class, the classes added in a
// fixed order; then the quantiles k = class (mod 4) of the point.  y2 null: no lpd; nq = 0: no quantiles.  Outputs in the call's point
// order; the points of a failed entry get NaN.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_warp_post(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                   const double *__restrict__ work, size_t work_stride, const int *__restrict__ kind,
                                                   const double *__restrict__ psi, const double *__restrict__ wv,
                                                   const double *__restrict__ y2, int nq, const double *__restrict__ zq,
                                                   double *__restrict__ zmean, double *__restrict__ zvar, double *__restrict__ quant,
                                                   double *__restrict__ lpd) {
    __shared__ double part[2][4][64];
    __shared__ double s_mean[64], s_sd[64];
    const PostTile T = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, c = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = T.e;
    const size_t pt = (size_t)T.p0 + lane;
    if (L.status[b] < 0) {
        const double nan = __builtin_nan("");
        if (lane < T.cnt) {
            if (c == 0) {
                zmean[pt] = nan;
                zvar[pt] = nan;
                if (y2) lpd[pt] = nan;
            }
            for (int k = c; k < nq; k += 4) quant[warp_quant_at(pt, nq, k)] = nan;
        }
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, Q = L.Q;
    const int pos = L.bpos ? L.bpos[b] : b;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride, *B = hyp + hyp_off_B(L);
    const double *w = wv + warp_vec_at(b, ld, 0);
    const double *Vf = work + (size_t)blockIdx.x * work_stride + (size_t)ld * 64;
    {
        double s1 = 0.0, s2 = 0.0;
        if (lane < T.cnt)
            for (int i = c; i < n; i += 4) {
                const double v = Vf[(size_t)i * 64 + lane];
                s1 += v * w[i];
                s2 += v * v;
            }
        part[0][c][lane] = s1;
        part[1][c][lane] = s2;
    }
    __syncthreads();
    if (tid < T.cnt) {
        const int m2 = meta2[pt];
        const double mean = ((part[0][0][tid] + part[0][1][tid]) + part[0][2][tid]) + part[0][3][tid];
        const double vv = ((part[1][0][tid] + part[1][1][tid]) + part[1][2][tid]) + part[1][3][tid];
        double kss = 0.0;
        for (int q = 0; q < Q; q++) kss += B[(size_t)q * D * D + m2 * D + m2];
        const double var = (kss - vv) + hyp[m2];
        zmean[pt] = mean;
        zvar[pt] = var;
        s_mean[tid] = mean;
        s_sd[tid] = sqrt(var);
        if (y2) {
            double gy = y2[pt], lj = 0.0;
            if (!kind || kind[m2] == MEDGP_WARP_SAS) warp_forward(warp_psi(psi, pos, D, m2), y2[pt], gy, lj);
            const double r = gy - mean;
            lpd[pt] = (-0.5 * log(2. * L.pi * var) - r * r / (2.0 * var)) + lj;
        }
    }
    __syncthreads();
    if (lane < T.cnt && nq > 0) {
        const int m2 = meta2[pt];
        const bool sas = !kind || kind[m2] == MEDGP_WARP_SAS;
        WarpPsi p{0.0, 0.0, 1.0, 0.0};
        if (sas) p = warp_psi(psi, pos, D, m2);
        for (int k = c; k < nq; k += 4) {
            const double zt = s_mean[lane] + zq[k] * s_sd[lane];
            quant[warp_quant_at(pt, nq, k)] = sas ? warp_inverse(p, zt) : zt;
        }
    }
}
