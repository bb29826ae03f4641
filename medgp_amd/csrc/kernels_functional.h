// kernels_functional.h -- posterior of LINEAR FUNCTIONALS g = sum_k a_k f_{m_k}(t_k) of the latent f: window means, change scores, contrasts.
//   ref: core/gp_regression.cpp:128-214 (predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
// The reference has no such output; the definition is tests/functional_ref.py.  With d = t_i - t_k (= -tau of the header's formulas):
//   K*_g[i] = sum_k a_k sum_q B_q[m_i, m_k] cos(w_q d) exp(-c_q d^2)      (terms in the caller's order, q inside)
//   V_g = L^-1 K*_g,  z = L^-1 y                                          (linearity: ONE solve column per functional)
//   fmean = V_g^T z,  fvar = q_g - V_g^T V_g                              (latent: no sigma^2)
//   q_g = sum_kl a_k a_l sum_q B_q[m_k, m_l] cos(w_q (t_k - t_l)) exp(-c_q (t_k - t_l)^2)       the prior variance of g
// Works on the state of k_posterior (kernels_posterior.h): L in Kmat, z, the diagonal-block inverses U_kk in Linv.
#pragma once
#include "medgp_dev.h"
#include "kernels_cholinv.h"     // v4d
#include "kernels_assemble.h"    // exp_neg
#include "kernels_posterior.h"   // the pieces of a point-prediction kernel
#include "inference_tables.h"    // PostTile

// The terms of a call as the device holds them, term x of the call (functional f owns terms [toff[f], toff[f + 1])):
//   m / t / a: covariate, time and weight;  fun: its functional;  c / s [x * Q + q]: cos / sin (w_q t_x), written by k_functional_prep;
//   rsum [x]: its row of the prior variance (below);  qg [f]: q_g.
struct FuncTerms {
    const int *toff, *fun, *m;
    const double *t, *a;
    double *c, *s, *rsum, *qg;
};

// ------------------------------------------------------------------------------------------
// Once per call and size class, one workgroup per tile of k_functional (the same tile table), for the terms of the tile's functionals --
// a contiguous range of the call's terms:
//   the tables cos / sin (w_q t_x), one sincos per (term, q): the only ones of the call;
//   the prior variance q_g of every functional, from the time DIFFERENCES themselves (cos (w_q (t_k - t_l)) and the envelope per pair:
//   the small q_g of a change score does not inherit the |w t| eps of the tables), by symmetry as
//     rsum[k] = a_k (a_k sum_q B_q[m_k, m_k] + 2 sum_{l < k} a_l sum_q B_q[m_k, m_l] cos(w_q d) exp(-c_q d^2)),   q_g = sum_k rsum[k]:
//   one thread per term (l ascending, q inside), then one thread per functional (k ascending): every sum is one sequential loop whose
//   order is the caller's term order, so q_g depends on the functional alone.  T^2 Q / 2 per functional, next to n T Q of K*.
// A failed entry is left alone (k_functional marks its functionals and reads nothing of this).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_functional_prep(MedgpDev L, const PostTile *__restrict__ tiles, FuncTerms F) {
    const PostTile T = tiles[blockIdx.x];
    const int b = T.e, tid = threadIdx.x, Q = L.Q, D = L.D;
    if (L.status[b] < 0) return;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L);
    const int x0 = F.toff[T.p0], x1 = F.toff[T.p0 + T.cnt];
    for (size_t e = tid; e < (size_t)(x1 - x0) * Q; e += 256) {
        const size_t x = x0 + e / Q;
        const int q = (int)(e % Q);
        double sn, cs;
        sincos(wq[q] * F.t[x], &sn, &cs);
        F.c[x * Q + q] = cs;
        F.s[x * Q + q] = sn;
    }
    for (int x = x0 + tid; x < x1; x += 256) {
        const int mk = F.m[x];
        const double tk = F.t[x], ak = F.a[x];
        double s = 0.0;
        for (int l = F.toff[F.fun[x]]; l < x; l++) {
            const double d = tk - F.t[l], dd = d * d;
            const double *Bq = B + mk * D + F.m[l];
            double kk = 0.0;
            for (int q = 0; q < Q; q++) kk += Bq[q * D * D] * (cos(wq[q] * d) * exp(-cq[q] * dd));
            s += F.a[l] * kk;
        }
        double kss = 0.0;
        for (int q = 0; q < Q; q++) kss += B[(q * D + mk) * D + mk];
        F.rsum[x] = ak * (ak * kss + 2.0 * s);
    }
    __syncthreads();   // the rows of the tile's functionals are written (by this workgroup)
    if (tid < T.cnt) {
        const int f = T.p0 + tid;
        double s = 0.0;
        for (int x = F.toff[f]; x < F.toff[f + 1]; x++) s += F.rsum[x];
        F.qg[f] = s;
    }
}

// K*_g of panel c0 in the accumulator layout of post_kstar, column c = functional c of the tile with its terms [k0[c], k1[c]) (an empty
// range: a functional without terms or a dead column, K* = 0).  Per element a loop over the column's terms in the caller's order and,
// inside, over q: one B_q[m_i, m_k], one exp_neg, cos (w_q d) from the entry's row tables cs / sn and the term tables (kstar_sep; no
// sincos here); the term's sum over q times a_k is added to the element.  The columns of a wave have different term counts: lanes idle
// on the short ones.  The sixteen elements of a lane are formed strip by strip in a rolled loop, four rows of one column at a time, and
// handed over through the lane's own places in Rs (which must be free; post_solve's layout), as comp_kstar.
struct FuncCols { int __attribute__((address_space(3))) *k0, *k1; };
__device__ __forceinline__ PostAcc func_kstar(const PostCtx C, const FuncCols tb, const FuncTerms F, int c0) {
    const int w = C.w, li = C.li, g = C.g, n = C.n, ld = C.ld, D = C.D, Q = C.Q;
#pragma unroll 1
    for (int cs = 0; cs < 4; cs++) {
        const int col = 16 * cs + li, k1 = tb.k1[col];
        double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (int k = tb.k0[col]; k < k1; k++) {
            const double tk = F.t[k], ak = F.a[k];
            const int mk = F.m[k];
            const double *tc = F.c + (size_t)k * Q, *ts = F.s + (size_t)k * Q;
            KStar s[4] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
#pragma unroll 1
            for (int q = 0; q < Q; q++) {
                const double cc = tc[q], sc = ts[q], cq = C.cq[q];
                const double *Bq = C.B + (size_t)q * D * D + mk;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = c0 + 16 * w + 4 * r + g;
                    if (i < n) {
                        const double d = C.t[i] - tk;
                        s[r] = kstar_sep<false>(s[r], Bq[C.meta[i] * D], C.csb[q * ld + i], C.snb[q * ld + i], cc, sc, 0.0, cq, d, d * d);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; r++) a[r] += ak * s[r].k;
        }
#pragma unroll
        for (int r = 0; r < 4; r++) C.Rs[(16 * w + 4 * r + g) * POST_LS + col] = a[r];
    }
    v4d acc[4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int cs = 0; cs < 4; cs++) acc[cs][r] = C.Rs[(16 * w + 4 * r + g) * POST_LS + 16 * cs + li];
    return PostAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

// ------------------------------------------------------------------------------------------
// The pieces of kernels_posterior.h on a tile of up to 64 FUNCTIONALS of one entry (any Q, one kernel): the 64 solve columns are the
// functionals (PostTile::p0 / cnt index functionals of the call),
//   R_k = K*_g,k - L[C_k, 0:c0] V[0:c0],   V_k = L_kk^-1 R_k
// and per panel, rows in order, column c: sum v z, sum v^2 (post_reduce, threads < 64).  The epilogue: thread c < cnt writes
// fmean = sum v z and fvar = q_g - sum v^2 as computed (no clamp); a functional without terms gets 0.0f / 0.0f (K* = 0, q_g = 0.0).
// A functional's outputs depend on the entry and its own term list alone, not on its tile, its column or the launch chunk.
// mean / var: the call's per-functional outputs; the prologue marks a failed entry's functionals there.
// __launch_bounds__(256, 3): the 52 KB of LDS admit three workgroups per CU, as k_components.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 3) k_functional(MedgpDev L, const PostTile *__restrict__ tiles, FuncTerms F, double *__restrict__ work,
                                                    size_t work_stride, float *__restrict__ mean, float *__restrict__ var) {
    constexpr int QT = 0;   // (the prologue's table shape; its colc / cols are not used: the term tables are in memory)
    __shared__ int colk0[64], colk1[64];
    POST_PROLOGUE(PostTile, 64, (void)0);
    const FuncCols tb{(int __attribute__((address_space(3))) *)colk0, (int __attribute__((address_space(3))) *)colk1};
    if (tid < 64) {   // (visible after the first barrier of the panel loop)
        const bool ok = tid < T.cnt;
        colk0[tid] = ok ? F.toff[T.p0 + tid] : 0;
        colk1[tid] = ok ? F.toff[T.p0 + tid + 1] : 0;
    }
    PostSums sum{0.0, 0.0, 0.0};   // column tid (tid < 64): sum v z, sum v^2
    for (int c0 = 0; c0 < npad; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done), the column tables are written
        post_solve(C, c0, post_sub_lv(C, c0, func_kstar(C, tb, F, c0)));
        sum = post_reduce<0>(C, c0, min(64, n - c0), sum);
    }
    if (tid < T.cnt) {
        const size_t f = (size_t)T.p0 + tid;
        mean[f] = (float)sum.s1;
        var[f] = (float)(F.qg[f] - sum.s2);
    }
}
