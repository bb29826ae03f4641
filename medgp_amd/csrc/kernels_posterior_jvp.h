// kernels_posterior_jvp.h -- directional derivatives of the posterior mean and variance in the hypers (medgp_posterior_jvp_batch).
// Works behind one pipeline run that left L (lower triangle of Kmat), U = L^-T (upper triangle of Linv) and alpha = K^-1 y of every
// entry.  With P = K^-1 = U U^T, Kdot = sum_k v_k dK/dtheta_k of the un-jittered K (k_fisher_prep, k_fisher_kdot) and, for test point j,
//   k_j     the column of K*,      w_j = P k_j,      u = Kdot alpha,
//   kdot_j  = sum_q e ((Bdot_q[m_i,m_j] + cv_q dt^2 B_q[m_i,m_j]) cos(w_q dt) + cmu_q dt B_q[m_i,m_j] sin(w_q dt)),  dt = t_i - t*_j,
//             e = exp(-c_q dt^2): the Kdot element without the noise term, from the same coefficient block,
//   kdot**_j = sum_q Bdot_q[m_j,m_j],      sigdot_j = noise[m_j] = 2 sigma^2_{m_j} v_sigma,m_j:
//   mean_j = k_j^T alpha                        dmean_j = kdot_j^T alpha - w_j^T u
//   var_j  = k**_j - k_j^T P k_j + sigma^2      dvar_j  = kdot**_j + sigdot_j - 2 kdot_j^T w_j + w_j^T Kdot w_j
// The reference has no such output: the definition is tests/posterior_jvp_truth.py.
//   k_pjvp_solve  once per call, one workgroup per tile of 64 points: K* panel by panel (pjvp_cross) into the tile's work rows, then
//                 V = U^T K* = L^-1 K* and W = U V = P K*, two triangular products on fp64 MFMA over the non-zero 64-blocks of U; W
//                 replaces K* in the work rows.  mean = sum K* alpha, var = k** - sum V^2 + sigma^2.
//   k_pjvp_u      per direction: u = Kdot alpha, one workgroup per 64 rows, four column classes summed in order and added in a fixed order
//   k_pjvp_dir    per direction, one workgroup per tile: for every 64-row panel I the Kdot* panel from the coefficient block (cos / sin of
//                 the difference from the tables of the rows and of the tile's points), Y_I = sum_J Kdot[I,J] W[J] on fp64 MFMA (Kdot
//                 from global memory, W through LDS), and per column, rows in order,
//                   s_a += kdot* alpha,  s_b += kdot* W,  s_c += W Y,  s_d += W u;
//                 dmean = s_a - s_d,  dvar = kdot** + sigdot - 2 s_b + s_c.
// No atomics.  An MFMA output element depends on its own row and column operands alone and every per-column sum is taken by one thread
// over the rows in order: the bits of (point, direction) depend on the patient, theta, that point and that direction, not on
// batch-mates, on the number of directions or the direction's position, on the other points, the tile or the column a point lands in,
// or on the launch chunk.
// MFMA operand layout and the accumulator layout of a 64 x 64 panel: kernels_posterior.h.
#pragma once
#include "kernels_posterior.h"
#include "kernels_fisher.h"
#include "pjvp_tables.h"

#define PJVP_MAX_Q 16   // the column tables of the tile kernels are sized for it (the entry point refuses Q > 16)

// acc = sum over k in [k0, k1) of A[i][k] X[k][0:64] for the rows i = c0 + 16 w .. of this wave; k0, k1 multiples of POST_KC.  X is a
// panel array [rows][64] in global memory, staged POST_KC rows at a time through Vs.  A comes from the matrix M of the entry:
//   MODE 0  A[i][k] = M[k][i], k <= i      (U^T: M = U, upper triangle)
//   MODE 1  A[i][k] = M[i][k], k >= i      (U)
//   MODE 2  A[i][k] = M[k][i]              (a symmetric matrix stored in full: Kdot)
// Rows and columns beyond n are taken as zeros, whatever M holds there.  Barriers: panel_product's (kernels_posterior.h).
template <int MODE>
__device__ __forceinline__ PostAcc pjvp_mm(const PostCtx C, const double *__restrict__ M, const double *X, int c0, int k0, int k1) {
    const int ld = C.ld, n = C.n;
    v4d acc[4];
#pragma unroll
    for (int cs = 0; cs < 4; cs++) acc[cs] = v4d{0.0, 0.0, 0.0, 0.0};
    const int i = c0 + 16 * C.w + C.li;
    const bool iok = i < n;
    panel_product<0>(acc, C.Vs, k0, k1, C.li, C.g,
                     [&](int kk) { panel_stage_rows(C.Vs, X, kk, 64, C.tid); },
                     [&](int k) {
                         bool ok = iok && k < n;
                         if constexpr (MODE == 0) ok = ok && k <= i;
                         if constexpr (MODE == 1) ok = ok && k >= i;
                         return ok ? (MODE == 1 ? M[(size_t)i * ld + k] : M[(size_t)k * ld + i]) : 0.0;
                     });
    return PostAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

// the wave's rows of a panel in the accumulator layout -> rows c0 .. of a panel array [rows][64] in global memory, zeros beyond n
__device__ __forceinline__ void pjvp_store(const PostCtx C, double *X, int c0, const PostAcc acc) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 16 * C.w + 4 * r + C.g;
#pragma unroll
        for (int cs = 0; cs < 4; cs++) X[(size_t)(c0 + row) * 64 + 16 * cs + C.li] = (c0 + row < C.n) ? acc.a[cs][r] : 0.0;
    }
}
// the same into Rs
__device__ __forceinline__ void pjvp_to_lds(const PostCtx C, int c0, const PostAcc acc) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 16 * C.w + 4 * r + C.g;
#pragma unroll
        for (int cs = 0; cs < 4; cs++) C.Rs[row * POST_LS + 16 * cs + C.li] = (c0 + row < C.n) ? acc.a[cs][r] : 0.0;
    }
}

// The prologue of the two tile kernels: the tile record, the thread's coordinates, the entry's sizes and pointers, the LDS buffers and
// all of it as the value `const PostCtx C` (a macro: FAILED may return from the kernel).
#define PJVP_PROLOGUE(FAILED) \
    __shared__ double Vs[POST_KC * POST_LS]; \
    __shared__ double Rs[64 * POST_LS]; \
    __shared__ double colc[PJVP_MAX_Q][64], cols[PJVP_MAX_Q][64]; \
    const PostTile T = tiles[blockIdx.x]; \
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4; \
    const int b = T.e; \
    if (L.status[b] < 0) { FAILED; } \
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, Q = L.Q, npad = medgp_roundup(n, 64); \
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride; \
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L); \
    const double *t = L.pt + (size_t)slot * L.pld; \
    const int *meta = L.pmeta + (size_t)slot * L.pld; \
    const double *csb = L.cs + (size_t)b * Q * ld, *snb = L.sn + (size_t)b * Q * ld; \
    const double *al = L.alpha + (size_t)b * ld, *U = L.Linv + (size_t)b * ld * ld; \
    const PostCtx C{tid, w, li, g, n, ld, D, Q, B, wq, cq, t, csb, snb, nullptr, nullptr, U, meta, nullptr, (ld_t *)Vs, (ld_t *)Rs, (ld_t *)colc, (ld_t *)cols}

// Column set-up of a tile: this lane's four points (point 16 ps + li: covariate, time, inside the tile's count; nothing is read of
// meta2 / t2 beyond the count) and the tile's tables colc / cols [q][point] = cos / sin (w_q t*), visible after the next barrier.
struct PjvpCols { int ms[4]; double ts[4]; bool ok[4]; };
__device__ __forceinline__ PjvpCols pjvp_columns(const PostCtx C, int p0, int cnt, const int *__restrict__ meta2, const double *__restrict__ t2) {
    PjvpCols c;
#pragma unroll
    for (int ps = 0; ps < 4; ps++) {
        const int pt = 16 * ps + C.li;
        c.ok[ps] = pt < cnt;
        c.ms[ps] = c.ok[ps] ? meta2[p0 + pt] : 0;
        c.ts[ps] = c.ok[ps] ? t2[p0 + pt] : 0.0;
    }
    if (C.tid < 64) {
        const double tc = C.tid < cnt ? t2[p0 + C.tid] : 0.0;
        for (int q = 0; q < C.Q; q++) {
            double sn, cs;
            sincos(C.wq[q] * tc, &sn, &cs);
            C.cols[q * 64 + C.tid] = sn;
            C.colc[q * 64 + C.tid] = cs;
        }
    }
    return c;
}

// The cross panel of rows c0 .. c0 + 63 against the tile's points in the accumulator layout, zeros beyond n and beyond the count:
//   DOT = false  K*:     sum_q e B_q[m_i,m_j] cd
//   DOT = true   Kdot*:  sum_q e ((Bdot_q[m_i,m_j] + cv_q dt^2 B_q[m_i,m_j]) cd + cmu_q dt B_q[m_i,m_j] sd)        (cf: the coefficient block)
// dt = t_i - t*_j, e = exp(-c_q dt^2), (cd, sd) = cos / sin (w_q dt) by the angle-difference identities from the tables of the rows
// (MedgpDev::cs / sn) and of the points, as k_fisher_kdot forms the Kdot element.  Any Q <= PJVP_MAX_Q: a run-time loop.
template <bool DOT>
__device__ __forceinline__ PostAcc pjvp_cross(const PostCtx C, const PjvpCols cl, const double *__restrict__ Bd, const double *__restrict__ cmu,
                                              const double *__restrict__ cv, int c0) {
    const int w = C.w, li = C.li, g = C.g, n = C.n, ld = C.ld, D = C.D;
    v4d acc[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = c0 + 16 * w + 4 * r + g;
        double a4[4] = {0.0, 0.0, 0.0, 0.0};
        if (i < n) {
            const double tr = C.t[i];
            const int mr = C.meta[i];
            for (int q = 0; q < C.Q; q++) {
                const double rc = C.csb[(size_t)q * ld + i], rsn = C.snb[(size_t)q * ld + i], c2n = -C.cq[q] * MEDGP_LOG2E;
                const double *Bq = C.B + (size_t)q * D * D + mr * D;
                double xm = 0.0, xv = 0.0;
                const double *Bdq = Bq;
                if constexpr (DOT) { xm = cmu[q]; xv = cv[q]; Bdq = Bd + (size_t)q * D * D + mr * D; }
#pragma unroll
                for (int ps = 0; ps < 4; ps++) {
                    if (cl.ok[ps]) {
                        const double dt = tr - cl.ts[ps], dd = dt * dt;
                        const double cc = C.colc[q * 64 + 16 * ps + li], sn = C.cols[q * 64 + 16 * ps + li];
                        const double cd = rc * cc + rsn * sn;
                        const double e = exp2_nonpos(c2n * dd);
                        const double bq = Bq[cl.ms[ps]];
                        if constexpr (DOT) {
                            const double sdf = rsn * cc - rc * sn;
                            a4[ps] += e * ((Bdq[cl.ms[ps]] + (xv * dd) * bq) * cd + ((xm * dt) * bq) * sdf);
                        } else a4[ps] += bq * (cd * e);
                    }
                }
            }
        }
#pragma unroll
        for (int ps = 0; ps < 4; ps++) acc[ps][r] = a4[ps];
    }
    return PostAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

// ------------------------------------------------------------------------------------------
// W = P K* of a tile of up to 64 test points of one entry, and the plug-in posterior.  The tile's work rows: [ld][64] K* -> W, then
// [ld][64] V behind them.  Three passes over the 64-row panels, each panel of a pass complete in global memory before the next pass
// reads it (pjvp_mm starts on a barrier).  A failed entry gets NaN in mean, var and all nvec derivative outputs of the tile's points.
// grid = the chunk's tiles.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pjvp_solve(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                    const double *__restrict__ t2, double *__restrict__ work, size_t work_stride, int nvec,
                                                    float *__restrict__ mean, float *__restrict__ var, double *__restrict__ dmean,
                                                    double *__restrict__ dvar) {
    PJVP_PROLOGUE(
        if (tid < T.cnt) {
            const size_t p = (size_t)T.p0 + tid;
            mean[p] = __builtin_nanf("");
            var[p] = __builtin_nanf("");
            for (int k = 0; k < nvec; k++) { dmean[p * nvec + k] = __builtin_nan(""); dvar[p * nvec + k] = __builtin_nan(""); }
        }
        return);
    double *Wk = work + (size_t)blockIdx.x * work_stride, *Vf = Wk + (size_t)ld * 64;
    const PjvpCols cl = pjvp_columns(C, T.p0, T.cnt, meta2, t2);
    __syncthreads();   // colc / cols are written
    for (int c0 = 0; c0 < npad; c0 += 64) pjvp_store(C, Wk, c0, pjvp_cross<false>(C, cl, nullptr, nullptr, nullptr, c0));
    double s1 = 0.0, s2 = 0.0;   // column tid (tid < 64)
    for (int c0 = 0; c0 < npad; c0 += 64) {
        const PostAcc acc = pjvp_mm<0>(C, U, Wk, c0, 0, c0 + 64);   // (behind its barriers: the previous panel's sums are taken)
        pjvp_store(C, Vf, c0, acc);
        pjvp_to_lds(C, c0, acc);
        __syncthreads();
        if (tid < 64) {
            const int rend = min(64, n - c0);
            for (int r = 0; r < rend; r++) {
                const double v = Rs[r * POST_LS + tid];
                s1 += Wk[(size_t)(c0 + r) * 64 + tid] * al[c0 + r];
                s2 += v * v;
            }
        }
    }
    for (int c0 = 0; c0 < npad; c0 += 64) pjvp_store(C, Wk, c0, pjvp_mm<1>(C, U, Vf, c0, c0, npad));   // (K* is dead: mean is summed)
    if (tid < T.cnt) {
        const size_t p = (size_t)T.p0 + tid;
        const int m2 = meta2[p];
        mean[p] = (float)s1;
        var[p] = (float)(post_kss(C, m2) - s2 + hyp[m2]);
    }
}

// u_i = sum_{k < n} Kdot[i][k] alpha_k (the symmetric Kdot read by columns: coalesced), zeros on the padding.  grid = (64-row blocks of
// the class's largest entry, entries); wave w sums the columns k = w (mod 4) in order, the four partial sums are added in a fixed order.
__global__ void __launch_bounds__(256) k_pjvp_u(MedgpDev L, const double *__restrict__ Kdot, double *__restrict__ uvec) {
    __shared__ double part[4][64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const int i = 64 * (int)blockIdx.x + lane;
    if (64 * (int)blockIdx.x >= npad) return;
    const double *Kd = Kdot + (size_t)b * ld * ld, *al = L.alpha + (size_t)b * ld;
    double s = 0.0;
    if (i < n)
        for (int k = w; k < n; k += 4) s += Kd[(size_t)k * ld + i] * al[k];
    part[w][lane] = s;
    __syncthreads();
    if (tid < 64) uvec[(size_t)b * ld + i] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

// ------------------------------------------------------------------------------------------
// One direction of a tile: reads W from the tile's work rows (k_pjvp_solve of the same chunk), the direction's coefficient block, Kdot
// and u.  Any Q <= PJVP_MAX_Q in one launch: the components are a run-time loop over the tables.  grid = the chunk's tiles.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pjvp_dir(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                  const double *__restrict__ t2, const double *__restrict__ work, size_t work_stride,
                                                  const double *__restrict__ coef, const double *__restrict__ Kdot,
                                                  const double *__restrict__ uvec, int nvec, int dir, double *__restrict__ dmean,
                                                  double *__restrict__ dvar) {
    PJVP_PROLOGUE(return);   // (k_pjvp_solve wrote the NaNs of a failed entry)
    const double *cf = coef + (size_t)b * L.hyp_stride;
    const double *Bd = cf + hyp_off_B(L), *cmu = cf + hyp_off_w(L), *cv = cf + hyp_off_c(L);
    const double *u = uvec + (size_t)b * ld, *Kd = Kdot + (size_t)b * ld * ld;
    const double *Wk = work + (size_t)blockIdx.x * work_stride;
    const PjvpCols cl = pjvp_columns(C, T.p0, T.cnt, meta2, t2);
    double sa = 0.0, sb = 0.0, sc = 0.0, sd = 0.0;   // column tid (tid < 64)
    for (int c0 = 0; c0 < npad; c0 += 64) {
        __syncthreads();   // the tables are written; Rs is free (the previous panel's sums are taken)
        pjvp_to_lds(C, c0, pjvp_cross<true>(C, cl, Bd, cmu, cv, c0));
        __syncthreads();
        const int rend = min(64, n - c0);
        if (tid < 64)
            for (int r = 0; r < rend; r++) {
                const double kd = Rs[r * POST_LS + tid];
                sa += kd * al[c0 + r];
                sb += kd * Wk[(size_t)(c0 + r) * 64 + tid];
            }
        const PostAcc y = pjvp_mm<2>(C, Kd, Wk, c0, 0, npad);   // (behind its barriers: the sums above are taken)
        pjvp_to_lds(C, c0, y);
        __syncthreads();
        if (tid < 64)
            for (int r = 0; r < rend; r++) {
                const double wv = Wk[(size_t)(c0 + r) * 64 + tid];
                sc += wv * Rs[r * POST_LS + tid];
                sd += wv * u[c0 + r];
            }
    }
    if (tid < T.cnt) {
        const size_t p = (size_t)T.p0 + tid;
        const int m2 = meta2[p];
        double kssd = 0.0;
        for (int q = 0; q < Q; q++) kssd += Bd[(size_t)q * D * D + m2 * D + m2];
        dmean[p * nvec + dir] = sa - sd;
        dvar[p * nvec + dir] = ((kssd + cf[m2]) - 2.0 * sb) + sc;
    }
}
