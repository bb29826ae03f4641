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
#include "kernels_posterior.h"   // the pieces of a point-prediction kernel
#include "inference_tables.h"    // TREND_TW (test points per tile), PostTile

// ------------------------------------------------------------------------------------------
// The pieces of kernels_posterior.h on a tile of up to TREND_TW = 32 test points of one entry: the 64-column block holds K* (values) in
// columns 0 .. 31 and K*' (slopes) in columns 32 .. 63 of the same 32 points (two value strips and two slope strips: point 16 ps + li
// sits in strip ps and in strip 2 + ps), so every L row fragment and every U_kk fragment loaded feeds both halves:
//   R_k = [K*_k | K*'_k] - L[C_k, 0:c0] [V | V'][0:c0],   [V_k | V'_k] = L_kk^-1 R_k
// and per column, rows in order: mean += v z, q += v^2 (columns < 32);  dmean += v' z, dq += v'^2 (columns >= 32);  x += v v'
// (column j with column j + 32 of the staged block).  The value columns go through the instructions of k_posterior's columns (the same
// functions; MFMA output columns are independent): mean and var come out with that kernel's bits.  A point's five outputs depend on
// its test point and the entry alone, not on its tile, its column or the launch chunk.
// For QT > 0 cos and sin of w_q (t_i - t*) come from the entry's row tables cs / sn and the tile's colc / cols (one sincos per point
// and component, one exp_neg per element and component); QT == 0 evaluates cos / sin / exp per element.
// The work rows of a tile are ld x 64 doubles, as k_posterior's.  No decomposition: neither the copy of K* nor its two barriers.
// The epilogue: threads 0 .. 31 write mean / var / cross of their point, threads 32 .. 63 dmean / dvar of point tid - 32.
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256) k_trend(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                               const double *__restrict__ t2, double *__restrict__ work, size_t work_stride,
                                               float *__restrict__ mean, float *__restrict__ var, float *__restrict__ dmean,
                                               float *__restrict__ dvar, float *__restrict__ cross) {
    POST_PROLOGUE(PostTile, TREND_TW, dmean[p] = __builtin_nanf(""); dvar[p] = __builtin_nanf(""); if (cross) cross[p] = __builtin_nanf(""));
    const PostCols<2> cl = post_columns<QT, TREND_TW>(C, T.p0, T.cnt, meta2, t2, true);
    PostSums sum{0.0, 0.0, 0.0};   // column tid (tid < 64): sum v z, sum v^2; tid < 32: sum v v'
    for (int c0 = 0; c0 < npad; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done)
        post_solve(C, c0, post_sub_lv(C, c0, post_kstar<QT, 2, true, false>(C, cl, c0)));
        sum = post_reduce<TREND_TW>(C, c0, min(64, n - c0), sum);
    }
    if (tid < T.cnt) {
        const size_t p = (size_t)T.p0 + tid;
        const int m2 = meta2[p];
        mean[p] = (float)sum.s1;
        var[p] = (float)(post_kss(C, m2) - sum.s2 + hyp[m2]);
        if (cross) cross[p] = (float)(0.0 - sum.sx);
    } else if (tid >= TREND_TW && tid - TREND_TW < T.cnt) {
        const size_t p = (size_t)T.p0 + tid - TREND_TW;
        const int m2 = meta2[p];
        double kdd = 0.0;
        for (int q = 0; q < Q; q++) kdd += B[q * D * D + m2 * D + m2] * (wq[q] * wq[q] + 2.0 * cq[q]);
        dmean[p] = (float)sum.s1;
        dvar[p] = (float)(kdd - sum.s2);
    }
}
