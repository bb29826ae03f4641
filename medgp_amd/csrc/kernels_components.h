// kernels_components.h -- posterior of every spectral COMPONENT f_q of the latent f = sum_q f_q at many test points.
//   ref: core/gp_regression.cpp:128-214 (predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
// The reference has no such output; the definition is tests/components_ref.py.  With d = t_i - t* (= -tau of the header's formulas):
//   K*_q[i] = B_q[m_i, m*] cos(w_q d) exp(-c_q d^2)                  (sum_q K*_q = K* of k_posterior)
//   V_q = L^-1 K*_q,  z = L^-1 y
//   cmean[q] = V_q^T z,  ccov[q, r] = delta_qr B_q[m*, m*] - V_q^T V_r  (latent: no sigma^2),  cvar[q] = ccov[q, q]
// Works on the state of k_posterior (kernels_posterior.h): L in Kmat, z, the diagonal-block inverses U_kk in Linv.
#pragma once
#include "medgp_dev.h"
#include "kernels_core.h"        // tile_decode
#include "kernels_cholinv.h"     // v4d
#include "kernels_assemble.h"    // exp_neg
#include "kernels_posterior.h"   // the pieces of a point-prediction kernel
#include "inference_tables.h"    // components_tw (test points per tile), PostTile

// Column set-up of a tile of cnt <= 64 / Q points: column c < cnt Q is (point c / Q, component c % Q), the others are dead (K* = 0).
// Everything a column needs sits in LDS tables indexed by the column (visible after the first barrier of the panel loop), so that no
// thread carries its four columns in registers over the panel loop: cos / sin (w_q t*) (one sincos per column), c_q, t*, m* and q.
struct CompTabs { ld_t *c, *s, *cq, *ts; int __attribute__((address_space(3))) *ms, *q; };   // q < 0: a dead column
__device__ __forceinline__ void comp_columns(const PostCtx C, const CompTabs tb, int p0, int cnt, const int *__restrict__ meta2,
                                             const double *__restrict__ t2) {
    if (C.tid < 64) {
        const int Q = C.Q, pt = C.tid / Q, q = C.tid - pt * Q;
        const bool ok = C.tid < cnt * Q;
        const double tc = ok ? t2[p0 + pt] : 0.0;
        double sn = 0.0, cs = 0.0;
        if (ok) sincos(C.wq[q] * tc, &sn, &cs);
        tb.s[C.tid] = sn;
        tb.c[C.tid] = cs;
        tb.cq[C.tid] = ok ? C.cq[q] : 0.0;
        tb.ts[C.tid] = tc;
        tb.ms[C.tid] = ok ? meta2[p0 + pt] : 0;
        tb.q[C.tid] = ok ? q : -1;
    }
}

// K*_k of panel c0 in the accumulator layout of post_kstar, every column with its own (m*, t*, q): ONE component per element (one
// B_q[m_i, m*], one exp_neg), cos (w_q d) from the entry's row tables cs / sn (k_prep fills them for every Q, on every route) and the
// tile's column tables, as kstar_sep.  The sixteen elements of a lane are formed strip by strip in a rolled loop and handed over
// through the lane's own places in Rs (which must be free; post_solve's layout): rolled, the loop holds one strip's loads at a time.
__device__ __forceinline__ PostAcc comp_kstar(const PostCtx C, const CompTabs tb, int c0) {
    const int w = C.w, li = C.li, g = C.g, n = C.n, ld = C.ld, D = C.D;
#pragma unroll 1
    for (int cs = 0; cs < 4; cs++) {
        const int col = 16 * cs + li, q = tb.q[col];
        const bool cok = q >= 0;
        const int qq = cok ? q : 0, ms = tb.ms[col];
        const double ts = tb.ts[col], cc = tb.c[col], sc = tb.s[col], cq = tb.cq[col];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * w + 4 * r + g, i = c0 + row;
            KStar k{0.0, 0.0};
            if (cok && i < n) {
                const double d = C.t[i] - ts, dd = d * d;
                k = kstar_sep<false>(k, C.B[(qq * D + C.meta[i]) * D + ms], C.csb[qq * ld + i], C.snb[qq * ld + i], cc, sc, 0.0, cq, d, dd);
            }
            C.Rs[row * POST_LS + col] = k.k;
        }
    }
    v4d acc[4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int cs = 0; cs < 4; cs++) acc[cs][r] = C.Rs[(16 * w + 4 * r + g) * POST_LS + 16 * cs + li];
    return PostAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

// pair e of a tile: point e / tri, components a > b of it (tri = Q (Q - 1) / 2 pairs per point); the two columns as a | b << 8
__device__ __forceinline__ int comp_pair(int e, int Q, int tri) {
    const int pt = e / tri;
    int I, J;
    tile_decode(e - pt * tri, I, J);   // I >= J: components I + 1 > J
    return (pt * Q + I + 1) | (pt * Q + J) << 8;
}

// ------------------------------------------------------------------------------------------
// The pieces of kernels_posterior.h on a tile of up to P = 64 / Q test points of one entry (any Q <= 64, one kernel): the 64-column
// block holds the Q component columns of every point, point after point,
//   R_k = [K*_q,k]_(point, q) - L[C_k, 0:c0] V[0:c0],   V_k = L_kk^-1 R_k
// and per panel, rows in order:  column (point, q): sum v z, sum v^2 (post_reduce, threads < 64);  with ccov, pair (point, q > r):
// sum v_q v_r from the staged block in Rs.  The cnt Q (Q - 1) / 2 pairs of a tile are dealt over the 256 threads (pair e to thread
// e % 256, at most eight per thread: 64 * 63 / 2 = 2016 pairs of one point at Q = 64); the running sum of pair e is double e behind the tile's ld x 64 work rows (P tri
// doubles: components_extra), read, carried over the panel's rows in order and written back by that one thread: every sum is one
// sequential loop over the rows, its bits do not depend on the thread or the columns it was dealt to.
// A point's outputs depend on its test point and the entry alone, not on its tile, its columns or the launch chunk.
// mean / var: the per-point buffers of the posterior call; the prologue marks a failed entry's points there, like its siblings, and the
// component outputs of those points get NaN next to them.  Nothing else is written to them and the call does not read them back.
// The epilogue: thread c < cnt Q writes cmean / cvar (and the diagonal of ccov, the same float) of column c, the pair threads write both
// triangles of ccov as 0.0 - sum.
// __launch_bounds__(256, 3): the 52 KB of LDS admit three workgroups per CU; held to three waves per SIMD the compiler keeps the MFMA
// accumulators in the 154 VGPRs it uses, without a spill (unbounded: 158 + 32 AGPRs, two waves per SIMD).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 3) k_components(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                    const double *__restrict__ t2, double *__restrict__ work, size_t work_stride,
                                                    float *__restrict__ mean, float *__restrict__ var, float *__restrict__ cmean,
                                                    float *__restrict__ cvar, float *__restrict__ ccov) {
    constexpr int QT = 0;   // (the prologue's table shape: one row of 64 columns; the component of a column is a run-time value)
    __shared__ double colq[64], colt[64];
    __shared__ int colm[64], colqi[64];
    POST_PROLOGUE(PostTile, 64, for (int q = 0; q < Q; q++) {
        cmean[p * Q + q] = __builtin_nanf("");
        cvar[p * Q + q] = __builtin_nanf("");
        if (ccov) for (int r = 0; r < Q; r++) ccov[(p * Q + q) * Q + r] = __builtin_nanf("");
    });
    const CompTabs tb{C.colc, C.cols, (ld_t *)colq, (ld_t *)colt, (int __attribute__((address_space(3))) *)colm, (int __attribute__((address_space(3))) *)colqi};
    comp_columns(C, tb, T.p0, T.cnt, meta2, t2);
    const int tri = Q * (Q - 1) / 2, npair = ccov ? T.cnt * tri : 0;
    double *psum = V + (size_t)ld * 64;   // [npair]
    for (int e = tid; e < npair; e += 256) psum[e] = 0.0;   // (read back by this thread alone)
    PostSums sum{0.0, 0.0, 0.0};   // column tid (tid < 64): sum v z, sum v^2
    for (int c0 = 0; c0 < npad; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done), the column tables are written
        post_solve(C, c0, post_sub_lv(C, c0, comp_kstar(C, tb, c0)));
        const int rend = min(64, n - c0);
        sum = post_reduce<0>(C, c0, rend, sum);
        for (int e = tid; e < npair; e += 256) {
            const int pc = comp_pair(e, Q, tri), ca = pc & 255, cb = pc >> 8;
            double s = psum[e];
            for (int r = 0; r < rend; r++) s += C.Rs[r * POST_LS + ca] * C.Rs[r * POST_LS + cb];
            psum[e] = s;
        }
    }
    if (tid < T.cnt * Q) {
        const int pt = tid / Q, q = tid - pt * Q;
        const size_t p = (size_t)T.p0 + pt, o = p * Q + q;
        const int m2 = meta2[p];
        const float v = (float)(B[(q * D + m2) * D + m2] - sum.s2);
        cmean[o] = (float)sum.s1;
        cvar[o] = v;
        if (ccov) ccov[o * Q + q] = v;
    }
    for (int e = tid; e < npair; e += 256) {
        const int pc = comp_pair(e, Q, tri), ca = pc & 255, cb = pc >> 8, pt = ca / Q, q = ca - pt * Q, r = cb - pt * Q;
        const size_t o = ((size_t)T.p0 + pt) * Q * Q;
        const float x = (float)(0.0 - psum[e]);
        ccov[o + (size_t)q * Q + r] = x;
        ccov[o + (size_t)r * Q + q] = x;
    }
}
