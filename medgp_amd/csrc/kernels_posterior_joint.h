// kernels_posterior_joint.h -- joint posterior of a patient's test points: covariance and sample paths.
//   C   = K** - V^T V + diag(sigma^2_{meta2})      (m x m per patient; V = L^-1 K*, the work rows k_posterior leaves)
//   y*_s = mean + chol(C) eps_s                     (sample path s, eps supplied by the caller)
// The diagonal of C is the `var` of GP_Regression::predict (ref: core/gp_regression.cpp:128-214: noise added once); the
// reference has no joint output -- the definition is the restatement in tests/posterior_joint_ref.py.
// Works behind k_posterior on a launch chunk of WHOLE patients: the work rows of all tiles of a patient are resident
// ([npad][64] doubles per tile of 64 points, rows >= n zero).
//   k_postcov<Q>  one workgroup per lower 64 x 64 tile pair (I >= J) of a patient: C_IJ, fp64 into Cbuf, float into cov
//   k_postfactor  one workgroup per patient: blocked left-looking Cholesky of C in place (lower; upper of the diagonal
//                 blocks zeroed), 64 x 64 diagonal blocks by diag_factor_wave
//   k_postdraw    one workgroup per (patient, 64-row block): samples = mean + Lc eps
// Every sum runs in a fixed order (no atomics) over operands that belong to the patient alone: a patient's outputs do not
// depend on its batch-mates, on the order of the patients or on the launch chunk.
// MFMA operand layout (v_mfma_f64_16x16x4_f64): A[li][g], B[g][li], C/D[4 r + g][li], li = lane & 15, g = lane >> 4.
#pragma once
#include "kernels_posterior.h"

#define PJ_BS 34   // LDS row stride (doubles) of the staged rows of L in k_postfactor

// JointPat (one patient of a joint call) and JointTile (one workgroup of k_postcov / k_postdraw): inference_tables.h

// acc = V_I^T V_J over the rows [0, npad) of two tiles' work rows ([npad][64] each) on fp64 MFMA, rows in order: the rows of V_J staged
// through Vs (POST_KC x POST_LS doubles of LDS) POST_KC at a time, those of V_I streamed from memory.  Wave w owns output rows
// 16 w .. 16 w + 15 and all four 16-column strips (acc[cs][r]: row 16 w + 4 r + g, column 16 cs + li).  Shared by k_postcov and
// k_funccov (kernels_functional_joint.h).  The sequence and the barrier contract are panel_product's (kernels_posterior.h): starts on
// a barrier, ends without one.  Kept as a loop of its own: on panel_product k_funccov measured 1.9 % slower.
__device__ __forceinline__ void pj_vtv(v4d (&acc)[4], const double *__restrict__ VI, const double *__restrict__ VJ, int npad, double *Vs,
                                       int tid, int w, int li, int g) {
#pragma unroll
    for (int cs = 0; cs < 4; cs++) acc[cs] = v4d{0.0, 0.0, 0.0, 0.0};
    const double *Ar = VI + 16 * w + li;
    for (int kk = 0; kk < npad; kk += POST_KC) {
        __syncthreads();   // Vs is free
#pragma unroll
        for (int x = tid; x < POST_KC * 64; x += 256) Vs[(x >> 6) * POST_LS + (x & 63)] = VJ[(size_t)(kk + (x >> 6)) * 64 + (x & 63)];
        double a[POST_KC / 4];
#pragma unroll
        for (int s = 0; s < POST_KC / 4; s++) a[s] = Ar[(size_t)(kk + 4 * s + g) * 64];
        __syncthreads();
#pragma unroll
        for (int s = 0; s < POST_KC / 4; s++)
#pragma unroll
            for (int cs = 0; cs < 4; cs++)
                acc[cs] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], Vs[(4 * s + g) * POST_LS + 16 * cs + li], acc[cs], 0, 0, 0);
    }
}

// ------------------------------------------------------------------------------------------
// C_IJ = K**_IJ - V_I^T V_J (+ sigma^2 on the diagonal; identity on rows / columns [m, mpad)).  acc = V_I^T V_J over the
// rows of V on fp64 MFMA: the rows of V_J staged through LDS POST_KC at a time, those of V_I streamed from memory (wave w
// owns output rows 16 w .. 16 w + 15 and all four 16-column strips).  K** in the separable form of k_posterior<Q> for
// Q <= 8 (cos / sin of the test times per component in LDS, one exp_neg per (pair, component)), per element as k_predict
// for the generic kernel.  A diagonal tile is mirrored from its lower triangle, an off-diagonal tile written to cov in
// both places from the same float: cov is exactly symmetric.
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ void __launch_bounds__(256) k_postcov(MedgpDev L, const JointPat *__restrict__ pats, const JointTile *__restrict__ pairs,
                                                 const int *__restrict__ meta2, const double *__restrict__ t2,
                                                 const double *__restrict__ work, size_t work_stride, double *__restrict__ Cbuf,
                                                 float *__restrict__ cov) {
    __shared__ double Vs[POST_KC * POST_LS];
    __shared__ double Rs[64 * POST_LS];
    static_assert(4 * (QT > 0 ? QT : 1) * 64 <= POST_KC * POST_LS, "the cos / sin tables reuse the staging buffer");
    typedef double tab_t[64];
    tab_t *rowc = (tab_t *)Vs, *rows = rowc + (QT > 0 ? QT : 1), *colc = rows + (QT > 0 ? QT : 1), *cols = colc + (QT > 0 ? QT : 1);   // after the product
    const JointTile T = pairs[blockIdx.x];
    const JointPat P = pats[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, m = P.m, mpad = medgp_roundup(m, 64), I = T.I, J = T.J;
    float *cv = cov ? cov + P.voff : nullptr;
    if (L.status[b] < 0) {
        if (cv)
            for (int x = tid; x < 64 * 64; x += 256) {
                const int i = 64 * I + (x >> 6), j = 64 * J + (x & 63);
                if (i < m && j < m) { cv[(size_t)i * m + j] = __builtin_nanf(""); cv[(size_t)j * m + i] = __builtin_nanf(""); }
            }
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot], D = L.D, npad = medgp_roundup(n, 64);
    const int Q = QT > 0 ? QT : L.Q;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L);
    const double *VI = work + (size_t)(P.tile0 + I) * work_stride, *VJ = work + (size_t)(P.tile0 + J) * work_stride;
    const int *m2 = meta2 + P.p0;
    const double *tt = t2 + P.p0;
    v4d acc[4];
    pj_vtv(acc, VI, VJ, npad, Vs, tid, w, li, g);
    // this lane's four columns
    int mc[4];
    double tc[4];
#pragma unroll
    for (int cs = 0; cs < 4; cs++) {
        const int j = 64 * J + 16 * cs + li;
        mc[cs] = j < m ? m2[j] : 0;
        tc[cs] = j < m ? tt[j] : 0.0;
    }
    __syncthreads();   // Vs is free: cos / sin (w_q t) of the tile's rows and columns
    if constexpr (QT > 0) {
        if (tid < 128) {
            const int c = tid & 63, p = (tid < 64 ? 64 * I : 64 * J) + c;
            const double tc = p < m ? tt[p] : 0.0;
#pragma unroll
            for (int q = 0; q < QT; q++) {
                double s, co;
                sincos(wq[q] * tc, &s, &co);
                if (tid < 64) { rows[q][c] = s; rowc[q][c] = co; } else { cols[q][c] = s; colc[q][c] = co; }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = 16 * w + 4 * r + g, i = 64 * I + row;
        const bool rin = i < m;
        const int mr = rin ? m2[i] : 0;
        const double tr = rin ? tt[i] : 0.0;
#pragma unroll
        for (int cs = 0; cs < 4; cs++) {
            const int col = 16 * cs + li, j = 64 * J + col;
            double v = (i == j) ? 1.0 : 0.0;   // identity padding
            if (rin && j < m) {
                const double d = tr - tc[cs], dd = d * d;
                const double *Bq = B + mr * D + mc[cs];
                KStar k{0.0, 0.0};   // k_posterior's element, the row factors from the LDS tables
                if constexpr (QT > 0) {
#pragma unroll
                    for (int q = 0; q < QT; q++)
                        k = kstar_sep<false>(k, Bq[q * D * D], rowc[q][row], rows[q][row], colc[q][col], cols[q][col], wq[q], cq[q], d, dd);
                } else {
                    for (int q = 0; q < Q; q++) k = kstar_gen<false>(k, Bq[q * D * D], wq[q], cq[q], d, dd);
                }
                v = k.k - acc[cs][r];
                if (i == j) v += hyp[mr];
            }
            Rs[row * POST_LS + col] = v;
        }
    }
    __syncthreads();
    double *Cp = Cbuf + P.coff;
    for (int x = tid; x < 64 * 64; x += 256) {
        const int r = x >> 6, c = x & 63;
        const double v = (I == J && c > r) ? Rs[c * POST_LS + r] : Rs[r * POST_LS + c];
        const int i = 64 * I + r, j = 64 * J + c;
        Cp[(size_t)i * mpad + j] = v;
        if (cv && i < m && j < m) cv[(size_t)i * m + j] = (float)v;
    }
    if (cv && I != J)   // the mirrored tile, rows of cov contiguous
        for (int x = tid; x < 64 * 64; x += 256) {
            const int c = x >> 6, r = x & 63;
            const int i = 64 * I + r, j = 64 * J + c;
            if (i < m && j < m) cv[(size_t)j * m + i] = (float)Rs[r * POST_LS + c];
        }
}

// ------------------------------------------------------------------------------------------
// Lc = chol(C) in place, one workgroup (4 waves) per patient, left-looking over the 64-wide block columns k:
//   R_Ik = C_Ik - L[I, 0:k] L[k, 0:k]^T     (fp64 MFMA; the rows of block k staged through LDS, those of block I streamed)
//   L_kk, X = L_kk^-1 from diag_factor_wave  (I == k; LAPACK's rule: a pivot <= 0 or NaN fails)
//   L_Ik = R_Ik X^T                          (fp64 MFMA from LDS)
// Wave w owns rows 16 w .. 16 w + 15 of block I.  No jitter loop: C >= sigma^2_min I in exact arithmetic.  A failed pivot
// (or a patient whose own factorisation failed) sets cstat[b] = -1.  The strict upper triangle of the diagonal blocks is
// written as zeros, so k_postdraw reads whole rows.  Few patients with thousands of points each are slow here (one
// workgroup): DESIGN 4.7b.
// ------------------------------------------------------------------------------------------
struct PostFactorSmem {
    union {                    // never live at the same time (a barrier separates the uses)
        double Dk[64][CI_S];   // R_kk -> L_kk, then R_Ik of the blocks below
        double Bs[64][PJ_BS];  // staged L[64 k + row][kk .. kk + POST_KC)
    };
    double Xk[64][CI_S];       // L_kk^-1 (lower, exact zeros above the diagonal)
    alignas(16) double dv[64 + 128];
    double logdet;
    int fail;
};
__global__ void __launch_bounds__(256) k_postfactor(MedgpDev L, const JointPat *__restrict__ pats, double *__restrict__ Cbuf,
                                                    int *__restrict__ cstat) {
    __shared__ PostFactorSmem sm;
    const JointPat P = pats[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    if (L.status[P.e] < 0) {
        if (tid == 0) cstat[P.b] = -1;
        return;
    }
    const int mpad = medgp_roundup(P.m, 64), nb = mpad / 64;
    double *Cp = Cbuf + P.coff;
    if (tid == 0) { sm.fail = 0; sm.logdet = 0.0; }
    for (int k = 0; k < nb; k++) {
        for (int I = k; I < nb; I++) {
            v4d acc[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double *src = Cp + (size_t)(64 * I + 16 * w + 4 * r + g) * mpad + 64 * k + li;
#pragma unroll
                for (int cs = 0; cs < 4; cs++) acc[cs][r] = src[16 * cs];
            }
            const double *Ar = Cp + (size_t)(64 * I + 16 * w + li) * mpad;
            for (int kk = 0; kk < 64 * k; kk += POST_KC) {
                __syncthreads();   // Bs is free
#pragma unroll
                for (int x = tid; x < 64 * POST_KC; x += 256)
                    sm.Bs[x / POST_KC][x % POST_KC] = Cp[(size_t)(64 * k + x / POST_KC) * mpad + kk + x % POST_KC];
                double a[POST_KC / 4];
#pragma unroll
                for (int s = 0; s < POST_KC / 4; s++) a[s] = Ar[kk + 4 * s + g];
                __syncthreads();
#pragma unroll
                for (int s = 0; s < POST_KC / 4; s++)
#pragma unroll
                    for (int cs = 0; cs < 4; cs++)
                        acc[cs] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], sm.Bs[16 * cs + li][4 * s + g], acc[cs], 0, 0, MFMA_NEGA);
            }
            __syncthreads();   // Dk is free (the previous block's solve has read it)
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int cs = 0; cs < 4; cs++) sm.Dk[16 * w + 4 * r + g][16 * cs + li] = acc[cs][r];
            __syncthreads();
            if (I == k) {
                if (w == 0) diag_factor_wave((ld_t *)&sm.Dk[0][0], (ld_t *)&sm.Xk[0][0], (ld_t *)sm.dv, (li_t *)&sm.fail, (ld_t *)&sm.logdet, lane);
                __syncthreads();
                if (sm.fail) {   // (uniform: read behind the barrier)
                    if (tid == 0) cstat[P.b] = -1;
                    return;
                }
                for (int x = tid; x < 64 * 64; x += 256) {
                    const int r = x >> 6, c = x & 63;
                    Cp[(size_t)(64 * k + r) * mpad + 64 * k + c] = (c <= r) ? sm.Dk[r][c] : 0.0;
                }
            } else {
                // L_Ik[i][j] = sum_{c <= j} R[i][c] X[j][c]
                v4d o[4];
#pragma unroll
                for (int cs = 0; cs < 4; cs++) o[cs] = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int s = 0; s < 16; s++) {
                    const double a = sm.Dk[16 * w + li][4 * s + g];
#pragma unroll
                    for (int cs = 0; cs < 4; cs++)
                        if (s < 4 * cs + 4) o[cs] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sm.Xk[16 * cs + li][4 * s + g], o[cs], 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    double *dst = Cp + (size_t)(64 * I + 16 * w + 4 * r + g) * mpad + 64 * k + li;
#pragma unroll
                    for (int cs = 0; cs < 4; cs++) dst[16 * cs] = o[cs][r];
                }
            }
        }
        __syncthreads();   // block column k is in memory for the steps that read it
    }
}

// ------------------------------------------------------------------------------------------
// samples[i][s] = mean_i + sum_{j <= i} Lc[i][j] eps[j][s] for the rows of one 64-row block of a patient: a lower-triangular
// (m x m) x (m x nsamp) product on fp64 MFMA, eps staged through LDS POST_KC rows at a time, the rows of Lc streamed.  mean_i
// is the fp64 sum k_posterior rounds to `mean` (V^T z over the rows in order), taken again from the resident work rows
// so that a sample carries one float rounding, not two.  Writes float.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_postdraw(MedgpDev L, const JointPat *__restrict__ pats, const JointTile *__restrict__ blks,
                                                  const double *__restrict__ work, size_t work_stride, const double *__restrict__ Cbuf,
                                                  const int *__restrict__ cstat, const double *__restrict__ eps, int nsamp,
                                                  float *__restrict__ samples) {
    __shared__ double Es[POST_KC * POST_LS];
    __shared__ double mu[64];
    const JointTile T = blks[blockIdx.x];
    const JointPat P = pats[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, m = P.m, mpad = medgp_roundup(m, 64), I = T.I;
    const int rows = min(64, m - 64 * I);
    float *out = samples + ((size_t)P.p0 + 64 * I) * nsamp;
    if (L.status[b] < 0 || cstat[P.b] < 0) {
        for (size_t x = tid; x < (size_t)rows * nsamp; x += 256) out[x] = __builtin_nanf("");
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot];
    if (tid < 64) {
        const double *V = work + (size_t)(P.tile0 + I) * work_stride, *zz = L.z + (size_t)b * L.ldn;
        double s = 0.0;
        for (int r = 0; r < n; r++) s += V[(size_t)r * 64 + tid] * zz[r];
        mu[tid] = s;
    }
    const double *Ar = Cbuf + P.coff + (size_t)(64 * I + 16 * w + li) * mpad;
    const double *ep = eps + (size_t)P.p0 * nsamp;
    for (int s0 = 0; s0 < nsamp; s0 += 64) {
        v4d acc[4];
#pragma unroll
        for (int cs = 0; cs < 4; cs++) acc[cs] = v4d{0.0, 0.0, 0.0, 0.0};
        panel_product<0>(acc, Es, 0, 64 * (I + 1), li, g,   // (its first barrier: mu is written)
                         [&](int kk) {
#pragma unroll
                             for (int x = tid; x < POST_KC * 64; x += 256) {
                                 const int j = kk + (x >> 6), s = s0 + (x & 63);
                                 Es[(x >> 6) * POST_LS + (x & 63)] = (j < m && s < nsamp) ? ep[(size_t)j * nsamp + s] : 0.0;
                             }
                         },
                         [&](int k) { return Ar[k]; });
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = 16 * w + 4 * r + g;
#pragma unroll
            for (int cs = 0; cs < 4; cs++) {
                const int s = s0 + 16 * cs + li;
                if (row < rows && s < nsamp) out[(size_t)row * nsamp + s] = (float)(mu[row] + acc[cs][r]);
            }
        }
    }
}
