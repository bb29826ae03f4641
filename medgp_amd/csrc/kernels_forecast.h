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
#include "kernels_posterior.h"   // the pieces of a point-prediction kernel; ForeTile (inference_tables.h)

// ------------------------------------------------------------------------------------------
// The pieces of kernels_posterior.h on k_posterior's tile (64 points, four value strips, the same K* forms; no decomposition: neither
// the copy of K* nor its two barriers) with
//   1. the tile record ForeTile and the panel loop cut at pend = ceil(pmax / 64) panels (rows >= pmax of V are never needed: row k of
//      V depends on rows <= k of K* only); a tile whose prefixes are all 0 touches no panel (nor fills colc / cols) and writes the prior,
//   2. the column reductions of column j taking rows < prefix[j] only: the row bound of post_reduce is per column, the
//      rows are summed in k_posterior's order.  K* and the MFMA loops are NOT masked (rows >= prefix[j] of column j are
//      formed and solved, and ignored): no branch inside them, and the value of V[k, j] does not depend on prefix[j],
//   3. the epilogue: lpd = -1/2 (log 2 pi + log var) - 1/2 (y2 - mean)^2 / var from the fp64 mean and var when y2 is
//      given, then both rounded to float.
// Bits: as k_posterior, every output of a column depends on that column's point, its prefix and the entry alone; with prefix >= n
// the column goes through the instructions of k_posterior's.
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256) k_forecast(MedgpDev L, const ForeTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                  const double *__restrict__ t2, const int *__restrict__ prefix,
                                                  const double *__restrict__ y2, double *__restrict__ work, size_t work_stride,
                                                  double log2pi, float *__restrict__ mean, float *__restrict__ var,
                                                  double *__restrict__ lpd) {
    POST_PROLOGUE(ForeTile, 64, if (y2) lpd[p] = __builtin_nan(""));
    const int pend = min(medgp_roundup(min(T.pmax, n), 64), npad);   // rows [0, pend): the tile's panels
    const PostCols<4> cl = post_columns<QT, 64>(C, T.p0, T.cnt, meta2, t2, pend > 0);
    const int pj = (tid < T.cnt) ? min(prefix[T.p0 + tid], n) : 0;   // column tid conditions on rows [0, pj)
    PostSums sum{0.0, 0.0, 0.0};                                      // column tid (tid < 64)
    for (int c0 = 0; c0 < pend; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done)
        post_solve(C, c0, post_sub_lv(C, c0, post_kstar<QT, 4, false, false>(C, cl, c0)));
        sum = post_reduce<0>(C, c0, min(64, pj - c0), sum);   // rows [c0, min(c0 + 64, pj)): the mask of the cut-off
    }
    if (tid < T.cnt) {
        const size_t p = (size_t)T.p0 + tid;
        const int m2 = meta2[p];
        const double v64 = post_kss(C, m2) - sum.s2 + hyp[m2];
        if (y2) {
            const double r = y2[p] - sum.s1;
            lpd[p] = -0.5 * (log2pi + log(v64)) - 0.5 * (r * r) / v64;
        }
        mean[p] = (float)sum.s1;
        var[p] = (float)v64;
    }
}
