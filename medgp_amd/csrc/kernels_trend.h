// kernels_trend.h -- posterior of the latent SLOPE f'_{m*}(t*) at many test points, next to the posterior of the value.
//   ref: core/gp_regression.cpp:128-214 (predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
// The reference has no such output; the definition is tests/trend_ref.py.  With d = t_i - t* (= -tau of the header's formulas):
//   K*[i]   = sum_q B_q[m_i, m*] cos(w_q d) exp(-c_q d^2)
//   K*'[i]  = sum_q B_q[m_i, m*] (w_q sin(w_q d) + 2 c_q d cos(w_q d)) exp(-c_q d^2)          (d/dt* of K*[i])
//   k''**   = sum_q B_q[m*, m*] (w_q^2 + 2 c_q)
//   V = L^-1 K*,  V' = L^-1 K*',  z = L^-1 y
//   mean = V^T z,  var = k** - sum V^2 + sigma^2_{m*}      (k_posterior's, bit for bit)
//   dmean = V'^T z,  dvar = k''** - sum V'^2,  cross = - sum V V'
// Works on the state of k_posterior (kernels_posterior.h): L in Kmat, z, the diagonal-block inverses U_kk in Linv.
#pragma once
#include "medgp_dev.h"
#include "kernels_cholinv.h"     // v4d
#include "kernels_assemble.h"    // exp_neg
#include "kernels_posterior.h"   // POST_KC, POST_LS
#include "inference_tables.h"    // TREND_TW (test points per tile), PostTile

// ------------------------------------------------------------------------------------------
// One workgroup (4 waves) per tile of up to TREND_TW = 32 test points of one entry.  The tile is k_posterior's 64-column block with
// columns 0 .. 31 holding K* (values) and columns 32 .. 63 holding K*' (slopes) of the same 32 points: the left-looking panel loop,
// its registers and its LDS are k_posterior's, and every L row fragment and every U_kk fragment loaded feeds both halves.
//   R_k = [K*_k | K*'_k] - L[C_k, 0:c0] [V | V'][0:c0]     (fp64 MFMA, earlier rows staged through LDS POST_KC at a time)
//   [V_k | V'_k] = L_kk^-1 R_k                              (fp64 MFMA with the stored U_kk)
// and per column, rows in order: mean += v z, q += v^2 (columns < 32);  dmean += v' z, dq += v'^2 (columns >= 32);  x += v v'
// (column j with column j + 32 of the staged block).  The value columns go through exactly the arithmetic of k_posterior
// (MFMA output columns are independent): mean and var come out with that kernel's bits.  A point's five outputs depend on its
// test point and the entry alone, not on its tile, its column or the launch chunk.
// For QT > 0 cos and sin of w_q (t_i - t*) come from the entry's row tables cs / sn and the tile's colc / cols (one sincos per point
// and component, one exp_neg per element and component); QT == 0 evaluates cos / sin / exp per element.
// The work rows of a tile are ld x 64 doubles, as k_posterior's.
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256) k_trend(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                               const double *__restrict__ t2, double *__restrict__ work, size_t work_stride,
                                               float *__restrict__ mean, float *__restrict__ var, float *__restrict__ dmean,
                                               float *__restrict__ dvar, float *__restrict__ cross) {
    __shared__ double Vs[POST_KC * POST_LS];
    __shared__ double Rs[64 * POST_LS];
    const PostTile T = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = T.e, slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, npad = medgp_roundup(n, 64);
    const int Q = QT > 0 ? QT : L.Q;
    if (L.status[b] < 0) {
        if (tid < T.cnt) {
            const size_t p = (size_t)T.p0 + tid;
            mean[p] = __builtin_nanf("");
            var[p] = __builtin_nanf("");
            dmean[p] = __builtin_nanf("");
            dvar[p] = __builtin_nanf("");
            if (cross) cross[p] = __builtin_nanf("");
        }
        return;
    }
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L);
    const double *t = L.pt + (size_t)slot * L.pld;
    const int *meta = L.pmeta + (size_t)slot * L.pld;
    const double *zz = L.z + (size_t)b * ld;
    const double *Lm = L.Kmat + (size_t)b * ld * ld, *U = L.Linv + (size_t)b * ld * ld;
    double *V = work + (size_t)blockIdx.x * work_stride;   // [npad][64]: columns 0 .. 31 V, 32 .. 63 V'
    // this lane's two points: point 16 ps + li sits in column strip ps (value) and strip 2 + ps (slope)
    int ms[2];
    double ts[2];
    bool ok[2];
#pragma unroll
    for (int ps = 0; ps < 2; ps++) {
        const int pt = 16 * ps + li;
        ok[ps] = pt < T.cnt;
        ms[ps] = ok[ps] ? meta2[T.p0 + pt] : 0;
        ts[ps] = ok[ps] ? t2[T.p0 + pt] : 0.0;
    }
    // cos / sin (w_q t*) of the tile's points (visible after the first barrier of the panel loop)
    __shared__ double colc[QT > 0 ? QT : 1][TREND_TW], cols[QT > 0 ? QT : 1][TREND_TW];
    const double *csb = L.cs + (size_t)b * Q * ld, *snb = L.sn + (size_t)b * Q * ld;
    if constexpr (QT > 0) {
        if (tid < TREND_TW) {
            const double tc = tid < T.cnt ? t2[T.p0 + tid] : 0.0;
#pragma unroll
            for (int q = 0; q < QT; q++) sincos(wq[q] * tc, &cols[q][tid], &colc[q][tid]);
        }
    }
    double s1 = 0.0, s2 = 0.0, sx = 0.0;   // column tid (tid < 64): sum v z, sum v^2; tid < 32: sum v v'
    for (int c0 = 0; c0 < npad; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done)
        // [K*_k | K*'_k] in this lane's accumulator layout
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
            for (int ps = 0; ps < 2; ps++) {
                double k = 0.0, k1 = 0.0;
                if (rin && ok[ps]) {
                    const double d = tr - ts[ps], dd = d * d;
                    const double *Bq = B + mr * D + ms[ps];
                    if constexpr (QT > 0) {   // cos / sin (w (t_i - t*)) from the row tables and the tile's column values
#pragma unroll
                        for (int q = 0; q < QT; q++) {
                            const double e = exp_neg(cq[q] * dd);
                            const double sd = rsn[q] * colc[q][16 * ps + li] - rc[q] * cols[q][16 * ps + li];
                            k += Bq[q * D * D] * ((rc[q] * colc[q][16 * ps + li] + rsn[q] * cols[q][16 * ps + li]) * e);
                            k1 += Bq[q * D * D] * ((wq[q] * sd + (2.0 * cq[q] * d) * (rc[q] * colc[q][16 * ps + li] + rsn[q] * cols[q][16 * ps + li])) * e);
                        }
                    } else {
                        for (int q = 0; q < Q; q++) {
                            const double e = exp(-cq[q] * dd);
                            k += Bq[q * D * D] * (cos(wq[q] * d) * e);
                            k1 += Bq[q * D * D] * ((wq[q] * sin(wq[q] * d) + (2.0 * cq[q] * d) * cos(wq[q] * d)) * e);
                        }
                    }
                }
                acc[ps][r] = k;
                acc[2 + ps][r] = k1;
            }
        }
        // R_k = [K*_k | K*'_k] - L[C_k, 0:c0] [V | V'][0:c0]
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
        // [V_k | V'_k] = L_kk^-1 R_k;  (L_kk^-1)[i][k] = U[c0 + k][c0 + i], k <= i: wave w needs k < 16 w + 16
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
                s1 += v * zz[c0 + r];
                s2 += v * v;
                if (tid < TREND_TW) sx += v * Rs[r * POST_LS + TREND_TW + tid];
            }
        }
    }
    if (tid < T.cnt) {
        const size_t p = (size_t)T.p0 + tid;
        const int m2 = meta2[p];
        double kss = 0.0;
        for (int q = 0; q < Q; q++) kss += B[q * D * D + m2 * D + m2];
        mean[p] = (float)s1;
        var[p] = (float)(kss - s2 + hyp[m2]);
        if (cross) cross[p] = (float)(0.0 - sx);
    } else if (tid >= TREND_TW && tid - TREND_TW < T.cnt) {
        const size_t p = (size_t)T.p0 + tid - TREND_TW;
        const int m2 = meta2[p];
        double kdd = 0.0;
        for (int q = 0; q < Q; q++) kdd += B[q * D * D + m2 * D + m2] * (wq[q] * wq[q] + 2.0 * cq[q]);
        dmean[p] = (float)s1;
        dvar[p] = (float)(kdd - s2);
    }
}
