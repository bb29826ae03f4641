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
// The staged 64-column product of every family behind the factorisation (users: DESIGN 4.7v):
//   acc += A[rows 16 w .. 16 w + 15 of a 64-row slab][k0 .. k1) B[k0 .. k1)][0 .. 63]     (NEG: the MFMA's negation bits; 1 subtracts)
// on v_mfma_f64_16x16x4_f64, k in order, in steps kk = k0, k0 + KC, ... < k1 of KC each (a last step that reaches beyond k1 is a full
// one: the callables mask).  Wave w owns 16 output rows and all four 16-column strips: acc[cs][r] is row 16 w + 4 r + g, column
// 16 cs + li.  B is a [k][64] operand that `stage(kk)` puts into Vs as
// Vs[r * POST_LS + c] = B[kk + r][c] (r < KC; called by all 256 threads; it masks what it must).  A is streamed: `aval(k)` returns this
// lane's value A[row 16 w + li][k].  acc starts from what the caller hands in.
// Barriers: every step STARTS on one (Vs is free, and what the workgroup stored to memory before the call or in the caller's previous
// step is visible to stage) and has one between staging and the MFMAs; the function ENDS WITHOUT one and leaves the last KC staged rows
// in Vs: the caller synchronises before it writes Vs, or anything that shares its memory, again.  With k0 >= k1 it does nothing, no
// barrier either.
// ------------------------------------------------------------------------------------------
template <int NEG, int KC = POST_KC, class LDS, class STAGE, class AVAL>
__device__ __forceinline__ void panel_product(v4d (&acc)[4], LDS *Vs, int k0, int k1, int li, int g, STAGE stage, AVAL aval) {
    for (int kk = k0; kk < k1; kk += KC) {
        __syncthreads();
        stage(kk);
        double a[KC / 4];
#pragma unroll
        for (int s = 0; s < KC / 4; s++) a[s] = aval(kk + 4 * s + g);
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KC / 4; s++)
#pragma unroll
            for (int cs = 0; cs < 4; cs++)
                acc[cs] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], Vs[(4 * s + g) * POST_LS + 16 * cs + li], acc[cs], 0, 0, NEG);
    }
}
// The row-major stage: Vs[r * POST_LS + c] = src[(k + r) * ldsrc + c], r < KC, c < 64 (src points at the operand's first column).
template <int KC = POST_KC, class LDS>
__device__ __forceinline__ void panel_stage_rows(LDS *Vs, const double *src, int k, size_t ldsrc, int tid) {
#pragma unroll
    for (int x = tid; x < KC * 64; x += 256) Vs[(x >> 6) * POST_LS + (x & 63)] = src[(size_t)(k + (x >> 6)) * ldsrc + (x & 63)];
}

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
// The pieces of a point-prediction kernel: k_posterior below, k_trend (kernels_trend.h), k_forecast (kernels_forecast.h).  Each is one
// workgroup (4 waves) per tile of test points of one entry and runs, for every 64-row panel k of the entry's factor, left-looking:
//   K*_k  formed on the fly (post_kstar),
//   R_k = K*_k - L[C_k, 0:c0] V[0:c0]      (post_sub_lv: fp64 MFMA; V rows of earlier panels staged through LDS, POST_KC at a time),
//   V_k = L_kk^-1 R_k                      (post_solve: fp64 MFMA with the stored U_kk; V_k to the work rows and to Rs),
//   per column, rows in order: sums of V_k z_k and V_k^2   (post_reduce).
// V lives in the tile's work rows (ld x 64 doubles) and is written once per panel.  Every output of a column depends on that column's
// test point and the entry alone (MFMA output elements are independent of the other columns, the reductions run in a fixed row order):
// the bits of a point do not depend on its batch-mates, its tile, its column or the launch chunk, and a column that two of the kernels
// both form goes through the same instructions in both.
// MFMA operand layout (v_mfma_f64_16x16x4_f64): A[li][g], B[g][li], C/D[4 r + g][li], li = lane & 15, g = lane >> 4.
// Wave w owns rows 16 w .. 16 w + 15 of a panel and all four 16-column strips of the tile.
// Values go in and out of the pieces by value (a local array handed over by reference is kept as one wide vector: kernels_wgrad.h).
// ------------------------------------------------------------------------------------------
struct PostCtx {
    int tid, w, li, g, n, ld, D, Q;
    const double *B, *wq, *cq, *t, *csb, *snb, *zz, *Lm, *U;
    const int *meta;
    double *V;
    ld_t *Vs, *Rs, *colc, *cols;   // LDS as ld_t: through generic pointers its addresses are not folded into offsets (k_trend<2>: 139 VGPRs, 2 waves per SIMD; so 135, 3)
};
struct PostAcc { v4d a[4]; };   // a[cs]: rows 16 w .. of the panel, columns 16 cs .. of the tile

// The prologue of a kernel <QT> with the arguments (MedgpDev L, const TILE *tiles, ..., work, work_stride, ..., mean, var, ...): the tile
// record T, the thread's coordinates, the entry's sizes and pointers, the LDS buffers Vs, Rs and colc / cols (cos / sin (w_q t*) of the
// tile's TW points) and, for the functions below, all of it again as the value `const PostCtx C`.  A failed entry gets NaN in mean and var
// of the tile's points (p) and in what MORE_NANS names, and the kernel returns (a macro: the return is the kernel's).
#define POST_PROLOGUE(TILE, TW, MORE_NANS) \
    __shared__ double Vs[POST_KC * POST_LS]; \
    __shared__ double Rs[64 * POST_LS]; \
    __shared__ double colc[QT > 0 ? QT : 1][TW], cols[QT > 0 ? QT : 1][TW]; \
    const TILE T = tiles[blockIdx.x]; \
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4; \
    const int b = T.e, slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, npad = medgp_roundup(n, 64); \
    const int Q = QT > 0 ? QT : L.Q; \
    if (L.status[b] < 0) { \
        if (tid < T.cnt) { \
            const size_t p = (size_t)T.p0 + tid; \
            mean[p] = __builtin_nanf(""); \
            var[p] = __builtin_nanf(""); \
            MORE_NANS; \
        } \
        return; \
    } \
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride; \
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L); \
    const double *t = L.pt + (size_t)slot * L.pld; \
    const int *meta = L.pmeta + (size_t)slot * L.pld; \
    const double *zz = L.z + (size_t)b * ld; \
    const double *Lm = L.Kmat + (size_t)b * ld * ld, *U = L.Linv + (size_t)b * ld * ld; \
    double *V = work + (size_t)blockIdx.x * work_stride;   /* [npad][64] */ \
    const double *csb = L.cs + (size_t)b * Q * ld, *snb = L.sn + (size_t)b * Q * ld; \
    const PostCtx C{tid, w, li, g, n, ld, D, Q, B, wq, cq, t, csb, snb, zz, Lm, U, meta, V, (ld_t *)Vs, (ld_t *)Rs, (ld_t *)colc, (ld_t *)cols}

// Column set-up of a tile of TW points (64, or TREND_TW): this lane's NP = TW / 16 points (point 16 ps + li: covariate, time, inside the
// tile's count) and, for QT > 0, the tile's tables colc / cols [q * TW + point] (visible after the first barrier of the panel loop;
// `live`: the tile has a panel that reads them).
template <int NP> struct PostCols { int ms[NP]; double ts[NP]; bool ok[NP]; };
template <int QT, int TW>
__device__ __forceinline__ PostCols<TW / 16> post_columns(const PostCtx C, int p0, int cnt, const int *__restrict__ meta2, const double *__restrict__ t2,
                                                          bool live) {
    PostCols<TW / 16> c;
#pragma unroll
    for (int ps = 0; ps < TW / 16; ps++) {
        const int pt = 16 * ps + C.li;
        c.ok[ps] = pt < cnt;
        c.ms[ps] = c.ok[ps] ? meta2[p0 + pt] : 0;
        c.ts[ps] = c.ok[ps] ? t2[p0 + pt] : 0.0;
    }
    if constexpr (QT > 0) {
        if (C.tid < TW && live) {
            const double tc = C.tid < cnt ? t2[p0 + C.tid] : 0.0;
#pragma unroll
            for (int q = 0; q < QT; q++) {
                double sn, cs;
                sincos(C.wq[q] * tc, &sn, &cs);
                C.cols[q * TW + C.tid] = sn;
                C.colc[q * TW + C.tid] = cs;
            }
        }
    }
    return c;
}

// One component of the K* element between an observation (row) and a test point (column), d = t_i - t*, dd = d^2, added to k:
//   k.k  += B_q cos(w_q d) exp(-c_q dd),   k.k1 += B_q (w_q sin(w_q d) + 2 c_q d cos(w_q d)) exp(-c_q dd)   (SLOPE: d/dt* of the first).
// kstar_sep: cos / sin (w_q d) from cos / sin (w_q t_i) = rc / rsn and cos / sin (w_q t*) = cc / sc, as k_assemble_t, one exp_neg;
// kstar_gen: cos, sin and exp per element, as k_predict.
struct KStar { double k, k1; };
template <bool SLOPE>
__device__ __forceinline__ KStar kstar_sep(KStar k, double Bq, double rc, double rsn, double cc, double sc, double w, double c, double d, double dd) {
    const double cd = rc * cc + rsn * sc, e = exp_neg(c * dd);
    k.k += Bq * (cd * e);
    if constexpr (SLOPE) k.k1 += Bq * ((w * (rsn * cc - rc * sc) + (2.0 * c * d) * cd) * e);
    return k;
}
template <bool SLOPE>
__device__ __forceinline__ KStar kstar_gen(KStar k, double Bq, double w, double c, double d, double dd) {
    const double e = exp(-c * dd);
    k.k += Bq * (cos(w * d) * e);
    if constexpr (SLOPE) k.k1 += Bq * ((w * sin(w * d) + (2.0 * c * d) * cos(w * d)) * e);
    return k;
}

// K*_k of panel c0 in this lane's accumulator layout: strips 0 .. NP - 1 the values of the lane's points and, with SLOPE, strips
// NP .. 2 NP - 1 their slopes.  COPY: the values also go to Rs (which must be free), in the layout of post_solve.
template <int QT, int NP, bool SLOPE, bool COPY>
__device__ __forceinline__ PostAcc post_kstar(const PostCtx C, const PostCols<NP> cl, int c0) {
    static_assert(NP * (SLOPE ? 2 : 1) == 4, "four 16-column strips");
    const int w = C.w, li = C.li, g = C.g, n = C.n, ld = C.ld, D = C.D;
    v4d acc[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 16 * w + 4 * r + g, i = c0 + row;
        const bool rin = i < n;
        const double tr = rin ? C.t[i] : 0.0;
        const int mr = rin ? C.meta[i] : 0;
        double rc[QT > 0 ? QT : 1], rsn[QT > 0 ? QT : 1];
        if constexpr (QT > 0) {
#pragma unroll
            for (int q = 0; q < QT; q++) { rc[q] = rin ? C.csb[q * ld + i] : 0.0; rsn[q] = rin ? C.snb[q * ld + i] : 0.0; }
        }
#pragma unroll
        for (int ps = 0; ps < NP; ps++) {
            KStar k{0.0, 0.0};
            if (rin && cl.ok[ps]) {
                const double d = tr - cl.ts[ps], dd = d * d;
                const double *Bq = C.B + mr * D + cl.ms[ps];
                if constexpr (QT > 0) {
#pragma unroll
                    for (int q = 0; q < QT; q++)
                        k = kstar_sep<SLOPE>(k, Bq[q * D * D], rc[q], rsn[q], C.colc[q * 16 * NP + 16 * ps + li], C.cols[q * 16 * NP + 16 * ps + li], C.wq[q], C.cq[q], d, dd);
                } else {
                    for (int q = 0; q < C.Q; q++) k = kstar_gen<SLOPE>(k, Bq[q * D * D], C.wq[q], C.cq[q], d, dd);
                }
            }
            acc[ps][r] = k.k;
            if constexpr (SLOPE) acc[NP + ps][r] = k.k1;
            if constexpr (COPY) C.Rs[row * POST_LS + 16 * ps + li] = k.k;
        }
    }
    return PostAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

// R_k = K*_k - L[C_k, 0:c0] V[0:c0]
__device__ __forceinline__ PostAcc post_sub_lv(const PostCtx C, int c0, const PostAcc in) {
    v4d acc[4] = {in.a[0], in.a[1], in.a[2], in.a[3]};
    const int arow = c0 + 16 * C.w + C.li;
    const bool aok = arow < C.n;
    const double *Lr = C.Lm + (size_t)arow * C.ld;
    panel_product<1>(acc, C.Vs, 0, c0, C.li, C.g,   // acc -= a b
                     [&](int kk) { panel_stage_rows(C.Vs, C.V, kk, 64, C.tid); },
                     [&](int k) { return aok ? Lr[k] : 0.0; });
    return PostAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

// R_k -> Rs (Rs must be free);  V_k = L_kk^-1 R_k;  V_k -> the work rows and Rs.  Ends on the barrier that makes V_k in Rs readable.
__device__ __forceinline__ void post_solve(const PostCtx C, int c0, const PostAcc acc) {
    const int w = C.w, li = C.li, g = C.g, n = C.n, ld = C.ld;
    ld_t *Rs = C.Rs;
    double *V = C.V;
    const double *U = C.U;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 16 * w + 4 * r + g;
#pragma unroll
        for (int cs = 0; cs < 4; cs++) Rs[row * POST_LS + 16 * cs + li] = (c0 + row < n) ? acc.a[cs][r] : 0.0;
    }
    __syncthreads();
    // (L_kk^-1)[i][k] = U[c0 + k][c0 + i], k <= i: wave w needs k < 16 w + 16
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
}

// Column tid (tid < 64) of V_k in Rs, rows [0, rend) in order: s1 += v z, s2 += v^2 and, for XW > 0 and tid < XW, sx += v v' with v' of
// column XW + tid.
struct PostSums { double s1, s2, sx; };
template <int XW>
__device__ __forceinline__ PostSums post_reduce(const PostCtx C, int c0, int rend, PostSums s) {
    if (C.tid < 64) {
        for (int r = 0; r < rend; r++) {
            const double v = C.Rs[r * POST_LS + C.tid];
            s.s1 += v * C.zz[c0 + r];
            s.s2 += v * v;
            if constexpr (XW > 0) {
                if (C.tid < XW) s.sx += v * C.Rs[r * POST_LS + XW + C.tid];
            }
        }
    }
    return s;
}

// k** = sum_q B_q[m*, m*]
__device__ __forceinline__ double post_kss(const PostCtx C, int m2) {
    double kss = 0.0;
    for (int q = 0; q < C.Q; q++) kss += C.B[q * C.D * C.D + m2 * C.D + m2];
    return kss;
}

// ------------------------------------------------------------------------------------------
// Posterior of a tile of up to 64 test points of one entry: four value strips, every panel of the factor, and next to the pieces above
// the per-covariate decomposition of the mean: K*_k is copied into Rs and, behind a barrier, summed into
//   part[d][j] += K*[r, j] alpha[r] (rows r of covariate d)
// by the threads of the columns while the others start on the product; one more barrier before R_k is staged (the decomposition has
// read Rs).  The copy and the two barriers do not depend on with_parts.
//   mean = sum V z,  var = k** - sum V^2 + sigma^2_{meta2}, as k_predict.
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256) k_posterior(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                   const double *__restrict__ t2, double *__restrict__ work, size_t work_stride,
                                                   int with_parts, int parts_lds, float *__restrict__ mean, float *__restrict__ var,
                                                   float *__restrict__ parts) {
    extern __shared__ double pacc_lds[];
    POST_PROLOGUE(PostTile, 64, if (with_parts) for (int d = 0; d < D; d++) parts[p * D + d] = __builtin_nanf(""));
    const double *al = L.alpha + (size_t)b * ld;
    double *pacc = parts_lds ? pacc_lds : V + (size_t)ld * 64;   // [D][64]
    if (with_parts && tid < 64)
        for (int d = 0; d < D; d++) pacc[d * 64 + tid] = 0.0;
    const PostCols<4> cl = post_columns<QT, 64>(C, T.p0, T.cnt, meta2, t2, true);
    PostSums sum{0.0, 0.0, 0.0};   // column tid (tid < 64)
    int pd = -1;                    // covariate of the current run of rows, and its partial sum (column tid)
    double pa = 0.0;
    for (int c0 = 0; c0 < npad; c0 += 64) {
        __syncthreads();   // Rs is free (previous panel's reductions done)
        PostAcc acc = post_kstar<QT, 4, false, true>(C, cl, c0);   // and a copy in Rs for the decomposition
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
        acc = post_sub_lv(C, c0, acc);
        __syncthreads();   // the decomposition has read Rs
        post_solve(C, c0, acc);
        sum = post_reduce<0>(C, c0, min(64, n - c0), sum);
    }
    if (tid < T.cnt) {
        const size_t p = (size_t)T.p0 + tid;
        const int m2 = meta2[p];
        mean[p] = (float)sum.s1;
        var[p] = (float)(post_kss(C, m2) - sum.s2 + hyp[m2]);
        if (with_parts) {
            if (pd >= 0) pacc[pd * 64 + tid] += pa;
            for (int d = 0; d < D; d++) parts[p * D + d] = (float)pacc[d * 64 + tid];
        }
    }
}
