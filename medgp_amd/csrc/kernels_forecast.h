// kernels_forecast.h -- rolling-origin forecasts: every test point is predicted from a LEADING block of its patient's
// observations (medgp_forecast_batch), all from the one factor of the whole patient.
//   ref: core/gp_regression.cpp:128-214 (GP_Regression::predict), main_one_test.cpp:269-300 (the "past" training sets)
// For a lower-triangular L the first p rows of V = L^-1 K* are L[0:p,0:p]^-1 K*[0:p], and L[0:p,0:p] is the factor of
// K[0:p,0:p]; likewise z[0:p] = L[0:p,0:p]^-1 y[0:p].  So the prediction of point j from the first p_j observations is
//   mean_j = sum_{k < p_j} V[k,j] z[k],   var_j = k** - sum_{k < p_j} V[k,j]^2 + sigma^2_{meta2_j}:
// k_posterior's column sums stopped at row p_j.  Works on the state of the same fit-only pipeline run as k_posterior (L in
// Kmat, z, the diagonal-block inverses U_kk in Linv), on the patient's CALLER-order copy: "the first p" is the caller's order.
#pragma once
#include "medgp_dev.h"
#include "kernels_cholinv.h"     // v4d
#include "kernels_assemble.h"    // exp_neg
#include "kernels_posterior.h"   // POST_TW, POST_KC, POST_LS; ForeTile (inference_tables.h)

// ------------------------------------------------------------------------------------------
// k_posterior (kernels_posterior.h: same workgroup shape, MFMA operand layout, left-looking panel loop, K* forms) with
//   1. the panel loop cut at ceil(pmax / 64) panels (rows >= pmax of V are never needed: row k of V depends on rows <= k of
//      K* only); a tile whose prefixes are all 0 touches no panel and writes the prior,
//   2. the column reductions of column j taking rows < prefix[j] only: the loop bound of the reduction is per column, the
//      rows are summed in k_posterior's order.  K* and the MFMA loops are NOT masked (rows >= prefix[j] of column j are
//      formed and solved, and ignored): no branch inside them, and the value of V[k, j] does not depend on prefix[j],
//   3. the epilogue: lpd = -1/2 (log 2 pi + log var) - 1/2 (y2 - mean)^2 / var from the fp64 mean and var when y2 is
//      given, then both rounded to float.
// Bits: as k_posterior, every output of a column depends on that column's point, its prefix and the entry alone.
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256) k_forecast(MedgpDev L, const ForeTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                  const double *__restrict__ t2, const int *__restrict__ prefix,
                                                  const double *__restrict__ y2, double *__restrict__ work, size_t work_stride,
                                                  double log2pi, float *__restrict__ mean, float *__restrict__ var,
                                                  double *__restrict__ lpd) {
    __shared__ double Vs[POST_KC * POST_LS];
    __shared__ double Rs[64 * POST_LS];
    const ForeTile T = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = T.e, slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D;
    const int Q = QT > 0 ? QT : L.Q;
    if (L.status[b] < 0) {
        if (tid < T.cnt) {
            const size_t p = (size_t)T.p0 + tid;
            mean[p] = __builtin_nanf("");
            var[p] = __builtin_nanf("");
            if (y2) lpd[p] = __builtin_nan("");
        }
        return;
    }
    const int pend = min(medgp_roundup(min(T.pmax, n), 64), medgp_roundup(n, 64));   // rows [0, pend): the tile's panels
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L);
    const double *t = L.pt + (size_t)slot * L.pld;
    const int *meta = L.pmeta + (size_t)slot * L.pld;
    const double *zz = L.z + (size_t)b * ld;
    const double *Lm = L.Kmat + (size_t)b * ld * ld, *U = L.Linv + (size_t)b * ld * ld;
    double *V = work + (size_t)blockIdx.x * work_stride;   // [pend][64]
    // this lane's four columns (one per 16-column strip)
    int ms[4];
    double ts[4];
    bool ok[4];
#pragma unroll
    for (int cs = 0; cs < 4; cs++) {
        const int col = 16 * cs + li;
        ok[cs] = col < T.cnt;
        ms[cs] = ok[cs] ? meta2[T.p0 + col] : 0;
        ts[cs] = ok[cs] ? t2[T.p0 + col] : 0.0;
    }
    // cos / sin (w_q t*) of the tile's columns (visible after the first barrier of the panel loop)
    __shared__ double colc[QT > 0 ? QT : 1][64], cols[QT > 0 ? QT : 1][64];
    const double *csb = L.cs + (size_t)b * Q * ld, *snb = L.sn + (size_t)b * Q * ld;
    if constexpr (QT > 0) {
        if (tid < 64 && pend > 0) {
            const double tc = tid < T.cnt ? t2[T.p0 + tid] : 0.0;
#pragma unroll
            for (int q = 0; q < QT; q++) sincos(wq[q] * tc, &cols[q][tid], &colc[q][tid]);
        }
    }
    const int pj = (tid < T.cnt) ? min(prefix[T.p0 + tid], n) : 0;   // column tid conditions on rows [0, pj)
    double msum = 0.0, qsum = 0.0;                                     // column tid (tid < 64)
    for (int c0 = 0; c0 < pend; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done)
        // K*_k in this lane's accumulator layout
        v4d acc[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * w + 4 * r + g, i = c0 + row;
            const bool rin = i < n;
            const double tr = rin ? t[i] : 0.0;
            const int mr = rin ? meta[i] : 0;
            double rc[QT > 0 ? QT : 1], rsn[QT > 0 ? QT : 1];
            if constexpr (QT > 0) {
#pragma unroll
                for (int q = 0; q < QT; q++) { rc[q] = rin ? csb[q * ld + i] : 0.0; rsn[q] = rin ? snb[q * ld + i] : 0.0; }
            }
#pragma unroll
            for (int cs = 0; cs < 4; cs++) {
                double k = 0.0;
                if (rin && ok[cs]) {
                    const double d = tr - ts[cs], dd = d * d;
                    const double *Bq = B + mr * D + ms[cs];
                    if constexpr (QT > 0) {   // cos(w (t_i - t*)) from the row tables and the tile's column values, as k_assemble_t
#pragma unroll
                        for (int q = 0; q < QT; q++)
                            k += Bq[q * D * D] * ((rc[q] * colc[q][16 * cs + li] + rsn[q] * cols[q][16 * cs + li]) * exp_neg(cq[q] * dd));
                    } else {
                        for (int q = 0; q < Q; q++) k += Bq[q * D * D] * (cos(wq[q] * d) * exp(-cq[q] * dd));
                    }
                }
                acc[cs][r] = k;
            }
        }
        // R_k = K*_k - L[C_k, 0:c0] V[0:c0]
        const int arow = c0 + 16 * w + li;
        const bool aok = arow < n;
        const double *Lr = Lm + (size_t)arow * ld;
        for (int kk = 0; kk < c0; kk += POST_KC) {
            __syncthreads();   // Vs is free
#pragma unroll
            for (int x = tid; x < POST_KC * 64; x += 256) Vs[(x >> 6) * POST_LS + (x & 63)] = V[(size_t)(kk + (x >> 6)) * 64 + (x & 63)];
            double a[POST_KC / 4];
#pragma unroll
            for (int s = 0; s < POST_KC / 4; s++) a[s] = aok ? Lr[kk + 4 * s + g] : 0.0;
            __syncthreads();
#pragma unroll
            for (int s = 0; s < POST_KC / 4; s++)
#pragma unroll
                for (int cs = 0; cs < 4; cs++)
                    acc[cs] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], Vs[(4 * s + g) * POST_LS + 16 * cs + li], acc[cs], 0, 0, 1);   // acc -= a b
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * w + 4 * r + g;
#pragma unroll
            for (int cs = 0; cs < 4; cs++) Rs[row * POST_LS + 16 * cs + li] = (c0 + row < n) ? acc[cs][r] : 0.0;
        }
        __syncthreads();
        // V_k = L_kk^-1 R_k;  (L_kk^-1)[i][k] = U[c0 + k][c0 + i], k <= i: wave w needs k < 16 w + 16
        v4d o[4];
#pragma unroll
        for (int cs = 0; cs < 4; cs++) o[cs] = v4d{0.0, 0.0, 0.0, 0.0};
        const int irow = 16 * w + li;
        const bool iok = c0 + irow < n;
        for (int s = 0; s < 4 * w + 4; s++) {
            const int k = 4 * s + g;
            const double a = (iok && k <= irow) ? U[(size_t)(c0 + k) * ld + c0 + irow] : 0.0;
#pragma unroll
            for (int cs = 0; cs < 4; cs++) o[cs] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Rs[k * POST_LS + 16 * cs + li], o[cs], 0, 0, 0);
        }
        __syncthreads();   // every wave has read R_k
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * w + 4 * r + g;
#pragma unroll
            for (int cs = 0; cs < 4; cs++) {
                const double v = (c0 + row < n) ? o[cs][r] : 0.0;
                Rs[row * POST_LS + 16 * cs + li] = v;
                V[(size_t)(c0 + row) * 64 + 16 * cs + li] = v;
            }
        }
        __syncthreads();
        if (tid < 64) {   // rows [c0, min(c0 + 64, pj)) of column tid, in order: the mask of the cut-off
            const int rend = min(64, pj - c0);
            for (int r = 0; r < rend; r++) {
                const double v = Rs[r * POST_LS + tid];
                msum += v * zz[c0 + r];
                qsum += v * v;
            }
        }
    }
    if (tid < T.cnt) {
        const size_t p = (size_t)T.p0 + tid;
        const int m2 = meta2[p];
        double kss = 0.0;
        for (int q = 0; q < Q; q++) kss += B[q * D * D + m2 * D + m2];
        const double v64 = kss - qsum + hyp[m2];
        if (y2) {
            const double r = y2[p] - msum;
            lpd[p] = -0.5 * (log2pi + log(v64)) - 0.5 * (r * r) / v64;
        }
        mean[p] = (float)msum;
        var[p] = (float)v64;
    }
}
