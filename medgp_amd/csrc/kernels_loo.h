// kernels_loo.h -- leave-one-out / leave-group-out predictive distribution of the training observations (medgp_loo_batch).
// Works behind one pipeline run that left U = L^-T (upper triangle of Linv) and alpha = K^-1 y of every entry.  For a held-out
// index set B (rows of the entry in its internal order, ascending) with M = (K^-1)_BB = U_B U_B^T:
//   cov(y_B | rest) = M^-1,   mean(y_B | rest) = y_B - M^-1 alpha_B,
//   log p(y_B | rest) = -1/2 alpha_B^T M^-1 alpha_B + 1/2 log det M - |B|/2 log 2 pi
// (Rasmussen & Williams 5.4.2 for |B| = 1; the block form is the Schur complement of K^-1).  The reference has no such output:
// the definition is the refit in tests/loo_ref.py.
//   k_loo_diag    one wave per singleton group: d_i = sum_{k >= i} U[i][k]^2, var = 1 / d_i, mean = y_i - alpha_i / d_i
//   k_loo_gram    one workgroup per (group, lower 64 x 64 tile pair): M_IJ from the gathered rows of U on fp64 MFMA
//   k_postfactor  (kernels_posterior_joint.h, unchanged) M = R R^T in place, one workgroup per group
//   k_loo_solve   per group: var_i = sum_k (R^-1)[k][i]^2 by a blocked forward solve of the identity, one workgroup per
//                 64-column tile, and one workgroup for w = R^-1 alpha_B, mean = y_B - R^-T w and lpd
// Every sum runs in a fixed order over operands that belong to the group alone: a group's outputs do not depend on its label,
// on the other groups, on the batch-mates or on the launch chunk.
// MFMA operand layout (v_mfma_f64_16x16x4_f64): A[li][g], B[g][li], C/D[4 r + g][li], li = lane & 15, g = lane >> 4.
#pragma once
#include "kernels_posterior_joint.h"

// LooSingle, LooRow, the JointPat / JointTile of a larger group and loo_block_doubles: inference_tables.h

// ------------------------------------------------------------------------------------------
// Singletons: row i of U is contiguous from its diagonal on; lane l takes the columns l, l + 64, ... of the row's 64-aligned
// window (coalesced), the 64 partial sums are added by a butterfly.  Columns left of the diagonal hold leftovers (medgp_dev.h)
// and are masked.  This is the whole of classic LOO: n^2 / 2 doubles read per patient.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_loo_diag(MedgpDev L, const LooSingle *__restrict__ tab, int count, double log2pi,
                                                  float *__restrict__ mean, float *__restrict__ var, double *__restrict__ lpd) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long x = (long long)blockIdx.x * 4 + w;
    if (x >= count) return;
    const LooSingle S = tab[x];
    const int b = S.e;
    if (L.status[b] < 0) return;   // (the outputs keep their NaN fill)
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, i = S.r;
    const double *ur = L.Linv + (size_t)b * ld * ld + (size_t)i * ld;
    double s = 0.0;
    for (int k = (i & ~63) + lane; k < n; k += 64) {
        const double u = (k >= i) ? ur[k] : 0.0;
        s += u * u;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) {
        const double a = L.alpha[(size_t)b * ld + i], y = L.py[(size_t)slot * L.pld + i];
        if (var) var[S.out] = (float)(1.0 / s);
        if (mean) mean[S.out] = (float)(y - a / s);
        if (lpd) lpd[S.g] = -0.5 * (a * a / s) + 0.5 * log(s) - 0.5 * log2pi;
    }
}

// ------------------------------------------------------------------------------------------
// M_IJ = sum_k U[r_I][k] U[r_J][k] for the rows r of tiles I >= J of a group's index list.  U is upper triangular and the list
// ascending, so the contraction starts at the first row index of tile I (rounded down to the staging step) and ends at n: no
// work on the structural zeros left of it.  The rows r_J are staged through LDS POST_KC columns at a time, the rows r_I streamed
// from memory (wave w owns output rows 16 w .. 16 w + 15 and all four 16-column strips).  Elements left of a row's diagonal
// and the rows of the padding are masked to zero; the block gets the identity on rows / columns [m, mpad).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_loo_gram(MedgpDev L, const JointPat *__restrict__ groups, const JointTile *__restrict__ pairs,
                                                  const LooRow *__restrict__ rows, double *__restrict__ Mbuf) {
    __shared__ double Vs[POST_KC * POST_LS];
    __shared__ int rI[64], rJ[64];
    const JointTile T = pairs[blockIdx.x];
    const JointPat P = groups[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, m = P.m, mpad = medgp_roundup(m, 64), I = T.I, J = T.J;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn;
    const double *U = L.Linv + (size_t)b * ld * ld;
    if (tid < 128) {
        const int c = tid & 63, p = 64 * (tid < 64 ? I : J) + c;
        (tid < 64 ? rI : rJ)[c] = p < m ? rows[P.p0 + p].r : -1;
    }
    __syncthreads();
    const int ra = rI[16 * w + li];
    const double *Ua = U + (size_t)(ra < 0 ? 0 : ra) * ld;
    v4d acc[4];
#pragma unroll
    for (int cs = 0; cs < 4; cs++) acc[cs] = v4d{0.0, 0.0, 0.0, 0.0};
    panel_product<0>(acc, Vs, rI[0] & ~(POST_KC - 1), n, li, g,   // (the last step is a full one too: both callables mask k >= n)
                     [&](int kk) {   // the rows r_J, gathered transposed
#pragma unroll
                         for (int x = tid; x < 64 * POST_KC; x += 256) {
                             const int c = x / POST_KC, k = kk + x % POST_KC, r = rJ[c];
                             Vs[(x % POST_KC) * POST_LS + c] = (r >= 0 && k >= r && k < n) ? U[(size_t)r * ld + k] : 0.0;
                         }
                     },
                     [&](int k) { return (ra >= 0 && k >= ra && k < n) ? Ua[k] : 0.0; });
    double *Mp = Mbuf + P.coff;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = 64 * I + 16 * w + 4 * r + g;
#pragma unroll
        for (int cs = 0; cs < 4; cs++) {
            const int j = 64 * J + 16 * cs + li;
            Mp[(size_t)i * mpad + j] = (i < m && j < m) ? acc[cs][r] : (i == j ? 1.0 : 0.0);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Behind k_postfactor (R lower in the group's block, exact zeros above the diagonal of the diagonal blocks, identity on the
// padding).  Two kinds of workgroup (4 waves):
//   column tile c (J == 0): the columns 64 c .. 64 c + 63 of X = R^-1 by loo_block_column_inverse (X_j kept in the group's second
//     block, the last block row not stored), var_i = sum_k X[k][i]^2, rows in order.
//   vector solves (J == 1): w = R^-1 alpha_B forward, u = R^-T w backward over the 64-row blocks (the block's off-diagonal
//     part by all four waves, partial sums added in a fixed order; the diagonal block by substitution across the lanes of
//     wave 0), then mean = y_B - u and lpd = -1/2 w^T w + sum_j log R_jj - m/2 log 2 pi.
// A group whose factorisation failed (gstat < 0) or whose patient has no factor keeps the NaN fill of its outputs.
// ------------------------------------------------------------------------------------------
struct LooSolveSmem {
    double Bs[POST_KC * POST_LS];   // staged rows of X_j
    double Dk[64 * POST_LS];      // right-hand side -> X_k
    double Rk[64 * POST_LS];      // R_kk
    double red[4][64];
    double rhs[64];
};
// X = R^-1 E_c, the columns 64 c .. 64 c + 63 of the inverse of the lower triangular R ([mpad][mpad], exact zeros above the diagonal of
// its diagonal blocks), block row by block row from the tile's own diagonal block:
//   X_k = R_kk^-1 (E_kc - sum_{c <= j < k} R_kj X_j)
// the sum by panel_product (the rows of X_j staged through sm.Bs from X, where the earlier steps stored them; those of R_kj streamed), then
// the right-hand side to sm.Dk and R_kk to sm.Rk, the 64 x 64 solve by substitution with one column per lane of wave 0, held in 64
// registers, and X_k from sm.Dk to X.  STORE_LAST: the last block row is stored too (nothing below reads it).  SUMSQ: returns, for
// tid < 64, the sum of x^2 down column 64 c + tid, rows in order (0 otherwise).  One workgroup of 4 waves; starts without a barrier (sm is
// free) and ends on the one behind the last solve, before the last store.
template <bool STORE_LAST, bool SUMSQ>
__device__ __forceinline__ double loo_block_column_inverse(LooSolveSmem &sm, const double *R, double *X, int mpad, int c, int tid, int w, int li, int g) {
    const int nb = mpad / 64;
    double csq = 0.0;
    for (int k = c; k < nb; k++) {
        v4d acc[4];
#pragma unroll
        for (int cs = 0; cs < 4; cs++) acc[cs] = v4d{0.0, 0.0, 0.0, 0.0};
        const double *Ar = R + (size_t)(64 * k + 16 * w + li) * mpad;
        panel_product<MFMA_NEGA>(acc, sm.Bs, 64 * c, 64 * k, li, g, [&](int kk) { panel_stage_rows(sm.Bs, X + 64 * c, kk, mpad, tid); }, [&](int j) { return Ar[j]; });
        __syncthreads();   // Dk / Rk are free
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int cs = 0; cs < 4; cs++) {
                const int row = 16 * w + 4 * r + g, col = 16 * cs + li;
                sm.Dk[row * POST_LS + col] = acc[cs][r] + ((k == c && row == col) ? 1.0 : 0.0);
            }
        for (int x = tid; x < 64 * 64; x += 256) sm.Rk[(x >> 6) * POST_LS + (x & 63)] = R[(size_t)(64 * k + (x >> 6)) * mpad + 64 * k + (x & 63)];
        __syncthreads();
        if (tid < 64) {   // R_kk x = d for column tid: x_l, then the rows below it
            double s[64];
#pragma unroll
            for (int i = 0; i < 64; i++) s[i] = sm.Dk[i * POST_LS + tid];
#pragma unroll
            for (int l = 0; l < 64; l++) {
                const double x = s[l] / sm.Rk[l * POST_LS + l];
                s[l] = x;
                if constexpr (SUMSQ) csq += x * x;
#pragma unroll
                for (int i = l + 1; i < 64; i++) s[i] -= sm.Rk[i * POST_LS + l] * x;
            }
#pragma unroll
            for (int i = 0; i < 64; i++) sm.Dk[i * POST_LS + tid] = s[i];
        }
        __syncthreads();
        if (STORE_LAST || k + 1 < nb)
            for (int x = tid; x < 64 * 64; x += 256) X[(size_t)(64 * k + (x >> 6)) * mpad + 64 * c + (x & 63)] = sm.Dk[(x >> 6) * POST_LS + (x & 63)];
    }
    return csq;
}
__global__ void __launch_bounds__(256) k_loo_solve(MedgpDev L, const JointPat *__restrict__ groups, const JointTile *__restrict__ jobs,
                                                   const LooRow *__restrict__ rows, double *__restrict__ Mbuf, const int *__restrict__ gstat,
                                                   double log2pi, float *__restrict__ mean, float *__restrict__ var, double *__restrict__ lpd) {
    __shared__ LooSolveSmem sm;
    const JointTile T = jobs[blockIdx.x];
    const JointPat P = groups[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, m = P.m, mpad = medgp_roundup(m, 64), nb = mpad / 64;
    if (L.status[b] < 0 || gstat[P.b] < 0) return;
    double *R = Mbuf + P.coff, *X = R + (size_t)mpad * mpad;
    const LooRow *rw = rows + P.p0;
    if (T.J == 0) {
        if (!var) return;
        const int c = T.I;
        const double csq = loo_block_column_inverse<false, true>(sm, R, X, mpad, c, tid, w, li, g);   // (tid < 64: column 64 c + tid)
        if (tid < 64 && 64 * c + tid < m) var[rw[64 * c + tid].out] = (float)csq;
        return;
    }
    // ---- the vector solves ----
    if (!mean && !lpd) return;
    const int slot = L.bslot[b], ld = L.ldn;
    const double *al = L.alpha + (size_t)b * ld, *yy = L.py + (size_t)slot * L.pld;
    double *wv = X + (size_t)mpad * mpad, *uv = wv + mpad;
    double wtw = 0.0, lgd = 0.0;   // (wave 0: this lane's rows of every block)
    for (int k = 0; k < nb; k++) {
        __syncthreads();   // rhs / Rk are free; w of the previous blocks is in memory
        for (int rr = 0; rr < 16; rr++) {
            const int row = 16 * w + rr, gi = 64 * k + row;
            const double *Rr = R + (size_t)gi * mpad;
            double s = 0.0;
            for (int j = lane; j < 64 * k; j += 64) s += Rr[j] * wv[j];
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
            if (lane == 0) sm.rhs[row] = (gi < m ? al[rw[gi].r] : 0.0) - s;
        }
        for (int x = tid; x < 64 * 64; x += 256) sm.Rk[(x >> 6) * POST_LS + (x & 63)] = R[(size_t)(64 * k + (x >> 6)) * mpad + 64 * k + (x & 63)];
        __syncthreads();
        if (tid < 64) {   // lane i holds row i
            double s = sm.rhs[lane];
            for (int l = 0; l < 64; l++) {
                const double x = __shfl(s, l) / sm.Rk[l * POST_LS + l];
                if (lane > l) s -= sm.Rk[lane * POST_LS + l] * x;
                if (lane == l) s = x;
            }
            wv[64 * k + lane] = s;
            wtw += s * s;
            lgd += log(sm.Rk[lane * POST_LS + lane]);   // (1 on the padding)
        }
    }
    if (mean)
        for (int k = nb - 1; k >= 0; k--) {
            __syncthreads();   // red / Rk are free; u of the blocks below is in memory
            {
                const int i = tid & 63, q = tid >> 6;
                double s = 0.0;
                for (int j = 64 * (k + 1) + q; j < mpad; j += 4) s += R[(size_t)j * mpad + 64 * k + i] * uv[j];
                sm.red[q][i] = s;
            }
            for (int x = tid; x < 64 * 64; x += 256) sm.Rk[(x >> 6) * POST_LS + (x & 63)] = R[(size_t)(64 * k + (x >> 6)) * mpad + 64 * k + (x & 63)];
            __syncthreads();
            if (tid < 64) {   // R_kk^T u = rhs: last row first
                double s = wv[64 * k + lane] - ((sm.red[0][lane] + sm.red[1][lane]) + (sm.red[2][lane] + sm.red[3][lane]));
                for (int l = 63; l >= 0; l--) {
                    const double x = __shfl(s, l) / sm.Rk[l * POST_LS + l];
                    if (lane < l) s -= sm.Rk[l * POST_LS + lane] * x;
                    if (lane == l) s = x;
                }
                uv[64 * k + lane] = s;
            }
        }
    __syncthreads();
    if (mean)
        for (int p = tid; p < m; p += 256) mean[rw[p].out] = (float)(yy[rw[p].r] - uv[p]);
    if (lpd && tid < 64) {
        for (int off = 32; off > 0; off >>= 1) { wtw += __shfl_xor(wtw, off); lgd += __shfl_xor(lgd, off); }
        if (lane == 0) lpd[P.b] = -0.5 * wtw + lgd - 0.5 * m * log2pi;
    }
}
