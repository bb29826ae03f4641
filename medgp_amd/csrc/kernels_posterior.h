// kernels_posterior.h -- batched posterior at many test points with the per-covariate decomposition of the mean.
//   ref: core/gp_regression.cpp:216-320 (GP_Regression::parsed_predict), :128-214 (predict),
//        kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram), :122-150 (self diagonal)
// Works on the state a fit-only pipeline run leaves (run_pipeline(..., store_ukk = true)): L in Kmat (lower triangle),
// z = L^-1 y, and the diagonal-block inverses U_kk = L_kk^-T in Linv (upper triangle of the diagonal blocks).  No inverse is formed.
#pragma once
#include "medgp_dev.h"
#include "kernels_cholinv.h"   // v4d
#include "kernels_assemble.h"  // exp_neg
#include "inference_tables.h"  // POST_TW (test points per tile = one workgroup), PostTile

#define POST_KC 32    // rows of V staged in LDS per step of the off-diagonal product
#define POST_LS 66    // LDS row stride (doubles) of the staged V rows and of the 64 x 64 block buffer
#define POST_PARTS_LDS_MAX_D 32   // up to this D the per-covariate accumulators of a tile live in LDS, beyond it in the work rows

// ------------------------------------------------------------------------------------------
// alpha = K^-1 y = L^-T z by blocked back substitution over the 64-wide panels, last panel first:
//   alpha_k = U_kk (z_k - sum_{j > k} L_jk^T alpha_j),   U_kk = L_kk^-T (stored by the factorisation)
// One workgroup per entry of the view.  Wave w sums the rows m = w (mod 4) of L below the panel (each row read as one
// coalesced 512-byte segment); the four partial sums are added in a fixed order.  Writes MedgpDev::alpha (0 beyond n).
// Only run when the caller asks for the decomposition.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_alpha(MedgpDev L) {
    __shared__ double part[4][64];
    __shared__ double rk[64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const double *Lm = L.Kmat + (size_t)b * ld * ld, *U = L.Linv + (size_t)b * ld * ld, *zz = L.z + (size_t)b * ld;
    double *al = L.alpha + (size_t)b * ld;
    for (int c0 = npad - 64; c0 >= 0; c0 -= 64) {
        const int i = c0 + lane;
        double s = 0.0;
        for (int m = c0 + 64 + w; m < n; m += 4) s += Lm[(size_t)m * ld + i] * al[m];   // (m > i: the lower triangle)
        part[w][lane] = s;
        __syncthreads();
        if (tid < 64) rk[tid] = (i < n) ? zz[i] - (((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]) : 0.0;
        __syncthreads();
        if (tid < 64) {   // (U_kk)[i][j] = U[c0 + i][c0 + j], j >= i
            double a = 0.0;
            if (i < n)
                for (int j = tid; j < 64 && c0 + j < n; j++) a += U[(size_t)i * ld + c0 + j] * rk[j];
            al[i] = a;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// Posterior of a tile of up to 64 test points of one entry (one workgroup, 4 waves).  For every 64-row panel k of the
// entry's factor, left-looking:
//   K*_k  formed on the fly (hyp offsets of k_predict; for Q <= 8 the separable form of k_assemble_t: cos w(t_i - t*) =
//         cs_i cos(w t*) + sn_i sin(w t*) from the entry's cos / sin tables, one exp_neg per component; the generic kernel
//         evaluates cos and exp per element as k_predict does), decomposed into the per-covariate parts
//         part[d][j] += K*[r, j] alpha[r] (rows r of covariate d),
//   R_k = K*_k - L[C_k, 0:c0] V[0:c0]      (fp64 MFMA; V rows of earlier panels staged through LDS, POST_KC at a time),
//   V_k = L_kk^-1 R_k                      (fp64 MFMA with the stored U_kk),
//   mean += V_k^T z_k,  q += sum V_k^2    (per column, rows in order).
// var = k** - q + sigma^2_{meta2}, as k_predict.  V lives in the tile's work rows (ld x 64 doubles) and is written once
// per panel.  Every output of a column depends on that column's test point and the entry alone (MFMA output elements
// are independent of the other columns, the reductions run in a fixed row order): the bits of a point do not depend on
// its batch-mates, its tile, its column or the launch chunk.
// MFMA operand layout (v_mfma_f64_16x16x4_f64): A[li][g], B[g][li], C/D[4 r + g][li], li = lane & 15, g = lane >> 4.
// Wave w owns rows 16 w .. 16 w + 15 of a panel and all four 16-column strips of the tile.
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256) k_posterior(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                   const double *__restrict__ t2, double *__restrict__ work, size_t work_stride,
                                                   int with_parts, int parts_lds, float *__restrict__ mean, float *__restrict__ var,
                                                   float *__restrict__ parts) {
    __shared__ double Vs[POST_KC * POST_LS];
    __shared__ double Rs[64 * POST_LS];
    extern __shared__ double pacc_lds[];
    const PostTile T = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = T.e, slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, npad = medgp_roundup(n, 64);
    const int Q = QT > 0 ? QT : L.Q;
    if (L.status[b] < 0) {
        if (tid < T.cnt) {
            const size_t p = (size_t)T.p0 + tid;
            mean[p] = __builtin_nanf("");
            var[p] = __builtin_nanf("");
            if (with_parts) for (int d = 0; d < D; d++) parts[p * D + d] = __builtin_nanf("");
        }
        return;
    }
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L);
    const double *t = L.pt + (size_t)slot * L.pld;
    const int *meta = L.pmeta + (size_t)slot * L.pld;
    const double *zz = L.z + (size_t)b * ld, *al = L.alpha + (size_t)b * ld;
    const double *Lm = L.Kmat + (size_t)b * ld * ld, *U = L.Linv + (size_t)b * ld * ld;
    double *V = work + (size_t)blockIdx.x * work_stride;   // [npad][64]
    double *pacc = parts_lds ? pacc_lds : V + (size_t)ld * 64;   // [D][64]
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
    if (with_parts && tid < 64)
        for (int d = 0; d < D; d++) pacc[d * 64 + tid] = 0.0;
    // cos / sin (w_q t*) of the tile's columns (visible after the first barrier of the panel loop)
    __shared__ double colc[QT > 0 ? QT : 1][64], cols[QT > 0 ? QT : 1][64];
    const double *csb = L.cs + (size_t)b * Q * ld, *snb = L.sn + (size_t)b * Q * ld;
    if constexpr (QT > 0) {
        if (tid < 64) {
            const double tc = tid < T.cnt ? t2[T.p0 + tid] : 0.0;
#pragma unroll
            for (int q = 0; q < QT; q++) sincos(wq[q] * tc, &cols[q][tid], &colc[q][tid]);
        }
    }
    double msum = 0.0, qsum = 0.0;   // column tid (tid < 64)
    int pd = -1;                      // covariate of the current run of rows, and its partial sum (column tid)
    double pa = 0.0;
    for (int c0 = 0; c0 < npad; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done)
        // K*_k in this lane's accumulator layout, and a copy in Rs for the decomposition
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
                Rs[row * POST_LS + 16 * cs + li] = k;
            }
        }
        __syncthreads();
        if (with_parts && tid < 64) {   // runs of equal covariate (the grouped copy: one run per covariate), rows in order
            const int rend = min(64, n - c0);
            for (int r = 0; r < rend; r++) {
                const int d = meta[c0 + r];
                if (d != pd) {
                    if (pd >= 0) pacc[pd * 64 + tid] += pa;
                    pd = d;
                    pa = 0.0;
                }
                pa += Rs[r * POST_LS + tid] * al[c0 + r];
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
        __syncthreads();   // the decomposition has read Rs
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
        if (tid < 64) {
            const int rend = min(64, n - c0);
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
        mean[p] = (float)msum;
        var[p] = (float)(kss - qsum + hyp[m2]);
        if (with_parts) {
            if (pd >= 0) pacc[pd * 64 + tid] += pa;
            for (int d = 0; d < D; d++) parts[p * D + d] = (float)pacc[d * 64 + tid];
        }
    }
}
