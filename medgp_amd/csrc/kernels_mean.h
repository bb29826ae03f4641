// kernels_mean.h -- a constant baseline per covariate, fixed or integrated out (medgp_mean_nlml_grad, medgp_mean_posterior_batch).
// Every other call assumes a zero mean.  Here y = H beta + f + noise with H[i, d] = [m_i = d] (n x D) and either
//   MEDGP_MEAN_FIXED     beta = b0, the reference's c_meanfunc_constMO (ref: mean/c_meanfunc_constMO.cpp, c_inference_exact.cpp:77-80,
//                        221-232; the scalar c_meanfunc_const is its D = 1 case), or
//   MEDGP_MEAN_MARGINAL  beta_d ~ N(b0_d, 1 / lam_d) integrated out in closed form (Rasmussen & Williams section 2.7; lam_d = 0: the flat
//                        prior, eq. 2.45): a GP with covariance K~ = K + H Lambda^-1 H^T, by Woodbury from the ONE factor of K.
// Works behind one unchanged pipeline run that left L, U = L^-T, z = L^-1 y and alpha.  With P = K^-1 = U U^T:
//   G = L^-1 H,  A = Lambda + G^T G,  w = L^-1 (y - H b0) = z - G b0,  c = G^T w,  delta = A^-1 c = beta^ - b0,
//   alpha~ = alpha - (P H) beta^,  Pm = (P H) chol(A)^-T  (Pm Pm^T = P H A^-1 H^T P),  W~ = P - Pm Pm^T - alpha~ alpha~^T,
//   nlml = 1/2 quad + 1/2 log|K| + 1/2 log|A| - 1/2 sum_{lam_d > 0} log lam_d + 1/2 (n - #{lam_d = 0}) log 2 pi,
//   quad = r0^T P r0 - c^T A^-1 c  EVALUATED AS  |w - G delta|^2 + sum_d lam_d delta_d^2   (the minimum over beta of the penalised
//          residual: a sum of squares, so nothing cancels where lam is small and the two terms of the first form are nearly equal),
//   d nlml / d theta_h = 1/2 tr(W~ dK/dtheta_h),   d nlml / d b0_d = -lam_d delta_d = -(H^T alpha~)_d.
// FIXED: delta = 0, beta^ = b0, no Pm, quad = |w|^2, dmean = -c.  The definition is tests/mean_truth.py.
//
//   k_mean_g      G: observations are grouped by covariate, so column d of G is the sum of the rows seg[d] .. seg[d + 1] of U, taken
//                 in order by one thread per (row, covariate); zeros on the padding rows and beyond column D
//   k_mean_small  one workgroup per entry: w, c, A and its Cholesky factor in LDS (packed lower triangles), Ti = chol(A)^-1, delta,
//                 beta^, A^-1, dmean, quad and the objective (-> scal[2], where k_epilogue's supplied-objective mode reads it).  A
//                 covariate without observations under the flat prior, or a failed pivot of A: status -1.  The program is
//                 fe_small_body, shared with k_basis_small (kernels_basis.h: any H with p <= 64 columns) behind a column policy
//   k_mean_panel  one workgroup per 64 rows: PH = U G on fp64 MFMA (k from the diagonal block on), then per row Pm = PH Ti^T and
//                 alpha~ = alpha - PH beta^, terms in order
//   k_mean_wgrad  k_wgrad's prologue and phase 1 on U, the accumulators continued through pv_phase1 over the one Pm panel with the
//                 staged operand negated (MARGINAL only), then k_wgrad's phases 2 and 3 with the nlml element on a view whose alpha is
//                 alpha~; diag(W~) leaves through wdiag.  W~ never reaches HBM.
//   k_slabsum, k_epilogue (kernels_core.h, unchanged; epi_mode = EPI_OBJECTIVE: the priors are added to the objective in scal[2])
//   k_mean_post   behind the unchanged k_pjvp_solve (V = L^-1 K* per tile of 64 points): the D x 64 tile G^T V on fp64 MFMA,
//                 r_j = e_{m*_j} - G^T V_j, mean_j = V_j^T z + r_j^T beta^, var_j = k** - V_j^T V_j + sigma^2 + |Ti r_j|^2 in fp64.  The
//                 program is fe_post_body, shared with k_basis_post behind the policy that gives a point's basis row
// No atomics; every sum in a fixed order over operands of the entry alone: an entry's bits depend neither on its batch-mates, nor on
// its position, the batch size or the launch chunk (with the route pinned, as everywhere); a point's neither on the other points nor
// on the tile column it lands in.
#pragma once
#include "kernels_posterior_vjp.h"
#include "mean_tables.h"

// ------------------------------------------------------------------------------------------
// grid = (64-row blocks of the class's largest entry, entries).  Lane = row, wave w owns the columns d = w (mod 4).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mean_g(MedgpDev L, double *__restrict__ G) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, npad = medgp_roundup(n, 64);
    const int r0 = 64 * (int)blockIdx.x;
    if (r0 >= npad) return;
    const int *seg = L.pseg + (size_t)slot * (D + 1);
    const double *U = L.Linv + (size_t)b * ld * ld;   // (L^-1)[i][j] = U[j][i], j <= i: the upper triangle
    const int i = r0 + lane;
    for (int d = w; d < MEAN_PW; d += 4) {
        double s = 0.0;
        if (d < D && i < n) {
            const int j1 = min(seg[d + 1], i + 1);
            for (int j = seg[d]; j < j1; j++) s += U[(size_t)j * ld + i];
        }
        G[mean_panel_at(b, ld, i, d)] = s;
    }
}

// ------------------------------------------------------------------------------------------
// The small step of the mean AND the basis calls (k_mean_small, k_basis_small: kernels_basis.h), one workgroup per entry.  D: the column
// count of H, an argument (the view's D stays the covariate count).  in = [b0 | lam] of the CALL in the caller's entry order
// (nbatch_call rows of D each), wvec and small: the class's part of the call's buffers (mean_tables.h with D columns).  The policy C:
//   row0(d)  the row at which the sums of c and A over column d start (it decides the four row classes of c, so it decides bits)
//   IMPROPER, improper(d, lam)  whether a column can be undetermined before any algebra (decided behind one __syncthreads_or)
//   SCALED_PIVOT, pivot_floor(d0, j)  pivot j of A fails when it is NaN or not above the floor; d0: the diagonal of A before the
//            factorisation, kept (s_d0) only where the floor depends on it
// (no __restrict__ on the two bodies: inlined, the pointers are the kernels' own restrict arguments)
// ------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ void fe_small_body(const MedgpDev &L, const C cols, const int D, const double *G, const double *in, int nbatch_call,
                                              int mode, double *wvec, double *small) {
    constexpr int TRI = MEAN_MAX_D * (MEAN_MAX_D + 1) / 2;
    __shared__ double Ap[TRI], Tp[TRI];
    __shared__ double s_b0[MEAN_MAX_D], s_lam[MEAN_MAX_D], s_c[MEAN_MAX_D], s_u[MEAN_MAX_D], s_dl[MEAN_MAX_D];
    __shared__ double s_d0[C::SCALED_PIVOT ? MEAN_MAX_D : 1];
    __shared__ double red[256];
    __shared__ int s_fail;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const int pos = L.bpos ? L.bpos[b] : b;   // the caller's row of this entry
    const bool marginal = mode == MEDGP_MEAN_MARGINAL;
    const double *z = L.z + (size_t)b * ld;
    double *wv = wvec + mean_vec_at(b, ld, 0);
    double *sm = small + (size_t)b * mean_small_stride(D);
    int bad = 0;
    for (int d = tid; d < D; d += 256) {
        const double lam = marginal ? in[(size_t)nbatch_call * D + (size_t)pos * D + d] : 0.0;
        s_b0[d] = in[(size_t)pos * D + d];
        s_lam[d] = lam;
        if constexpr (C::IMPROPER)
            if (marginal && cols.improper(d, lam)) bad = 1;   // nothing determines beta_d
    }
    if (tid == 0) s_fail = 0;
    if constexpr (C::IMPROPER) {
        if (__syncthreads_or(bad)) {
            if (tid == 0) L.status[b] = -1;
            return;
        }
    } else
        __syncthreads();
    // w = z - G b0, columns in order
    for (int i = tid; i < npad; i += 256) {
        double s = 0.0;
        if (i < n) {
            s = z[i];
            for (int d = 0; d < D; d++) s -= G[mean_panel_at(b, ld, i, d)] * s_b0[d];
        }
        wv[i] = s;
    }
    __syncthreads();
    // c = G^T w: four row classes per column, added in a fixed order
    {
        const int d = tid & 63, part = tid >> 6;
        double s = 0.0;
        if (d < D)
            for (int i = cols.row0(d) + part; i < n; i += 4) s += G[mean_panel_at(b, ld, i, d)] * wv[i];
        red[tid] = s;
        __syncthreads();
        if (tid < D) s_c[tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
        __syncthreads();
    }
    double logA = 0.0;   // thread 0: sum log diag chol(A) = 1/2 log|A|
    if (marginal) {
        // A = Lambda + G^T G, lower triangle, one thread per element, rows in order
        for (int idx = tid; idx < D * (D + 1) / 2; idx += 256) {
            int d, e;
            tile_decode(idx, d, e);
            double s = 0.0;
            for (int i = cols.row0(d); i < n; i++) s += G[mean_panel_at(b, ld, i, d)] * G[mean_panel_at(b, ld, i, e)];
            Ap[mean_tri_at(d, e)] = (d == e) ? s_lam[d] + s : s;
            if constexpr (C::SCALED_PIVOT)
                if (d == e) s_d0[d] = s_lam[d] + s;
        }
        __syncthreads();
        // right-looking Cholesky in place; a pivot fails when it is NaN or not above the policy's floor
        for (int j = 0; j < D; j++) {
            if (tid == 0) {
                const double piv = Ap[mean_tri_at(j, j)];
                if (!(piv > cols.pivot_floor(s_d0, j))) s_fail = 1;
                Ap[mean_tri_at(j, j)] = sqrt(piv);
            }
            __syncthreads();
            if (s_fail) break;   // (workgroup-uniform: read behind the barrier)
            const double ljj = Ap[mean_tri_at(j, j)];
            for (int i = j + 1 + tid; i < D; i += 256) Ap[mean_tri_at(i, j)] = Ap[mean_tri_at(i, j)] / ljj;
            __syncthreads();
            const int m = D - 1 - j;   // trailing rows j + 1 .. D - 1
            for (int idx = tid; idx < m * (m + 1) / 2; idx += 256) {
                int r, k;
                tile_decode(idx, r, k);
                const int i2 = j + 1 + r, k2 = j + 1 + k;
                Ap[mean_tri_at(i2, k2)] = Ap[mean_tri_at(i2, k2)] - Ap[mean_tri_at(i2, j)] * Ap[mean_tri_at(k2, j)];
            }
            __syncthreads();
        }
        if (s_fail) {
            if (tid == 0) L.status[b] = -1;
            return;
        }
        // Ti = chol(A)^-1 by forward substitution, one thread per column
        if (tid < D) {
            const int j = tid;
            for (int i = j; i < D; i++) {
                double s = (i == j) ? 1.0 : 0.0;
                for (int k = j; k < i; k++) s -= Ap[mean_tri_at(i, k)] * Tp[mean_tri_at(k, j)];
                Tp[mean_tri_at(i, j)] = s / Ap[mean_tri_at(i, i)];
            }
        }
        __syncthreads();
        if (tid < D) {   // u = Ti c
            double s = 0.0;
            for (int e = 0; e <= tid; e++) s += Tp[mean_tri_at(tid, e)] * s_c[e];
            s_u[tid] = s;
        }
        __syncthreads();
        if (tid < D) {   // delta = Ti^T u
            double s = 0.0;
            for (int k = tid; k < D; k++) s += Tp[mean_tri_at(k, tid)] * s_u[k];
            s_dl[tid] = s;
        }
        if (tid == 0)
            for (int d = 0; d < D; d++) logA += log(Ap[mean_tri_at(d, d)]);
        __syncthreads();
    } else {
        for (int d = tid; d < D; d += 256) s_dl[d] = 0.0;
        __syncthreads();
    }
    // the small outputs
    for (int d = tid; d < D; d += 256) {
        sm[mean_off_beta(D) + d] = s_b0[d] + s_dl[d];
        sm[mean_off_dmean(D) + d] = marginal ? -(s_lam[d] * s_dl[d]) : -s_c[d];
        sm[mean_off_delta(D) + d] = s_dl[d];
    }
    for (int idx = tid; idx < D * D; idx += 256) {
        const int d = idx / D, e = idx - d * D;
        double ti = 0.0, cv = 0.0;
        if (marginal) {
            if (e <= d) ti = Tp[mean_tri_at(d, e)];
            for (int k = max(d, e); k < D; k++) cv += Tp[mean_tri_at(k, d)] * Tp[mean_tri_at(k, e)];   // A^-1 = Ti^T Ti
        }
        sm[mean_off_ti(D) + idx] = ti;
        sm[mean_off_cov(D) + idx] = cv;
    }
    // quad = |w - G delta|^2 + sum lam delta^2: per thread the rows tid, tid + 256, ... in order, then one fixed tree
    {
        double s = 0.0;
        for (int i = tid; i < n; i += 256) {
            double r = wv[i];
            if (marginal)
                for (int d = 0; d < D; d++) r -= G[mean_panel_at(b, ld, i, d)] * s_dl[d];
            s += r * r;
        }
        red[tid] = s;
        __syncthreads();
        for (int off = 128; off > 0; off >>= 1) {
            if (tid < off) red[tid] += red[tid + off];
            __syncthreads();
        }
    }
    if (tid == 0) {
        double quad = red[0], loglam = 0.0;
        int nfree = 0;
        if (marginal)
            for (int d = 0; d < D; d++) {
                quad += s_lam[d] * (s_dl[d] * s_dl[d]);
                if (s_lam[d] > 0.0) loglam += log(s_lam[d]);
                else nfree++;
            }
        // (scal[0] = sum log diag L = 1/2 log|K|, as k_epilogue reads it)
        L.scal[b * 4 + 2] = quad / 2.0 + L.scal[b * 4 + 0] + logA - loglam / 2.0 + (n - nfree) * log(2. * L.pi) / 2.0;
    }
}

// the indicator columns: column d of G is zero above row seg[d]; a covariate without observations under the flat prior is improper;
// LAPACK's failure rule (a pivot <= 0 or NaN)
struct MeanSmallCols {
    static constexpr bool IMPROPER = true, SCALED_PIVOT = false;
    const int *seg;   // the entry's D + 1 segment starts
    __device__ __forceinline__ int row0(int d) const { return seg[d]; }
    __device__ __forceinline__ bool improper(int d, double lam) const { return lam == 0.0 && seg[d + 1] == seg[d]; }
    __device__ __forceinline__ double pivot_floor(const double *, int) const { return 0.0; }
};
// grid = the class's entries
__global__ void __launch_bounds__(256) k_mean_small(MedgpDev L, const double *__restrict__ G, const double *__restrict__ in, int nbatch_call,
                                                    int mode, double *__restrict__ wvec, double *__restrict__ small) {
    fe_small_body(L, MeanSmallCols{L.pseg + (size_t)L.bslot[blockIdx.x] * (L.D + 1)}, L.D, G, in, nbatch_call, mode, wvec, small);
}

// ------------------------------------------------------------------------------------------
// grid = (64-row blocks of the class's largest entry, entries); wave w owns the rows 16 w .. of the block, all column tiles below D.
// MFMA operand layout as WG_CHUNK_MFMA (kernels_wgrad.h): lane (li, g) gives A[row li][k g] and B[k g][col li], accumulator element r is
// C[row 4 r + g][col li].  A = U from global memory (masked to its upper triangle and to n), B = G from global memory.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_mean_panel(MedgpDev L, const double *__restrict__ G, const double *__restrict__ small, int mode,
                                                    double *__restrict__ PH, double *__restrict__ Pm, double *__restrict__ atilde) {
    constexpr int TRI = MEAN_MAX_D * (MEAN_MAX_D + 1) / 2;
    __shared__ double PHs[64][65];
    __shared__ double Tp[TRI];
    __shared__ double s_beta[MEAN_MAX_D];
    const int b = blockIdx.y, I = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, npad = medgp_roundup(n, 64);
    if (64 * I >= npad) return;
    const bool marginal = mode == MEDGP_MEAN_MARGINAL;
    const double *sm = small + (size_t)b * mean_small_stride(D);
    const double *U = L.Linv + (size_t)b * ld * ld, *al = L.alpha + (size_t)b * ld;
    for (int d = tid; d < D; d += 256) s_beta[d] = sm[mean_off_beta(D) + d];
    if (marginal)
        for (int idx = tid; idx < D * (D + 1) / 2; idx += 256) {
            int d, e;
            tile_decode(idx, d, e);
            Tp[mean_tri_at(d, e)] = sm[mean_off_ti(D) + (size_t)d * D + e];
        }
    v4d acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[ct] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int row = 64 * I + 16 * w + li, nct = (D + 15) / 16;
    for (int k = mean_panel_k0(I); k < npad; k += 4) {
        const int kk = k + g;
        const double a = (row < n && kk < n && kk >= row) ? U[(size_t)row * ld + kk] : 0.0;
#pragma unroll
        for (int ct = 0; ct < 4; ct++)
            if (ct < nct) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, G[mean_panel_at(b, ld, kk, 16 * ct + li)], acc[ct], 0, 0, 0);
    }
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int rl = 16 * w + 4 * r + g;
            PHs[rl][16 * ct + li] = acc[ct][r];
            PH[mean_panel_at(b, ld, 64 * I + rl, 16 * ct + li)] = acc[ct][r];
        }
    __syncthreads();
    const int rl = tid >> 2, qd = tid & 3, i = 64 * I + rl;
    if (marginal)
        for (int d = qd; d < MEAN_PW; d += 4) {
            double s = 0.0;
            if (d < D)
                for (int e = 0; e <= d; e++) s += PHs[rl][e] * Tp[mean_tri_at(d, e)];
            Pm[mean_panel_at(b, ld, i, d)] = s;
        }
    if (qd == 0) {
        double s = 0.0;
        for (int d = 0; d < D; d++) s += PHs[rl][d] * s_beta[d];
        atilde[mean_vec_at(b, ld, i)] = (i < n) ? al[i] - s : 0.0;
    }
}

// the staged operand of the panel pass negated: acc -= Pm[I rows] Pm[J rows]^T
struct MeanNegHook {
    __device__ __forceinline__ v2d operator()(v2d x, int, int) const { return -x; }
};

// ------------------------------------------------------------------------------------------
// W~ tile + gradient block reductions of a class's entries.  L: a view whose alpha is alpha~.  k1: the k range of the panel pass
// (mean_wgrad_k1; 0 in FIXED mode: no panel pass).  QT / Q0 as in k_wgrad: 8 < Q <= 16 takes two launches, each forming the tile again.
// ------------------------------------------------------------------------------------------
// (workgroups per SIMD promised to the compiler: kernels_hess.h's rule, as k_pvjp_wgrad)
constexpr int mean_wgrad_minwaves(int QT) { return QT >= 8 ? 2 : WG_MINWAVES; }
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, mean_wgrad_minwaves(QT)) k_mean_wgrad(MedgpDev L, const double *__restrict__ Pm, int k1, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<WgElemNlml, QT>];
    WG_PROLOGUE(false);
    const double *U = L.Linv + (size_t)T.b * T.ld * T.ld;
    WgAcc acc = wg_phase1<true>(smem, T, U, 64 * T.I, WgNoHook());
    const double *Pb = Pm + mean_panel_at(T.b, T.ld, 0, 0);
    acc = pv_phase1(acc, smem, T, Pb, 64 * T.I, Pb, 64 * T.J, k1, T.I == T.J, MeanNegHook());
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, WgElemNlml());
}

// ------------------------------------------------------------------------------------------
// The posterior step of the mean AND the basis calls (k_mean_post, k_basis_post: kernels_basis.h), one workgroup per tile of the chunk
// (k_pjvp_solve of the same chunk left V behind the first panel of every tile's work rows).  ncol: the column count of H, an
// argument -- the view's D stays the covariate count, which k** and the noise line need.  Wave w owns the rows d = 16 w .. of the
// ncol x 64 tile G^T V; mean / var: fp64, the call's point order.  The policy's h(pt, m2, d): entry d of the basis row of point pt.
// ------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ void fe_post_body(const MedgpDev &L, const C cols, const int ncol, const PostTile *tiles, const int *meta2,
                                             const double *work, size_t work_stride, const double *G, const double *small, int mode,
                                             double *mean, double *var) {
    __shared__ double Cs[64][65];
    __shared__ double part[2][4][64];
    const PostTile T = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = T.e;
    if (L.status[b] < 0) {
        if (tid < T.cnt) { mean[(size_t)T.p0 + tid] = __builtin_nan(""); var[(size_t)T.p0 + tid] = __builtin_nan(""); }
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, D = L.D, Q = L.Q, npad = medgp_roundup(n, 64);
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride, *B = hyp + hyp_off_B(L);
    const double *z = L.z + (size_t)b * ld;
    const double *Vf = work + (size_t)blockIdx.x * work_stride + (size_t)ld * 64;
    const double *sm = small + (size_t)b * mean_small_stride(ncol);
    v4d acc[4];
#pragma unroll
    for (int cs = 0; cs < 4; cs++) acc[cs] = (v4d){0.0, 0.0, 0.0, 0.0};
    if (16 * w < ncol)   // wave-uniform
        for (int k = 0; k < npad; k += 4) {
            const int kk = k + g;
            const double a = G[mean_panel_at(b, ld, kk, 16 * w + li)];
#pragma unroll
            for (int cs = 0; cs < 4; cs++) acc[cs] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Vf[(size_t)kk * 64 + 16 * cs + li], acc[cs], 0, 0, 0);
        }
#pragma unroll
    for (int cs = 0; cs < 4; cs++)
#pragma unroll
        for (int r = 0; r < 4; r++) Cs[16 * w + 4 * r + g][16 * cs + li] = acc[cs][r];
    // the zero-mean moments: four row classes per column, added in a fixed order
    {
        double s1 = 0.0, s2 = 0.0;
        if (lane < T.cnt)
            for (int i = w; i < n; i += 4) {
                const double v = Vf[(size_t)i * 64 + lane];
                s1 += v * z[i];
                s2 += v * v;
            }
        part[0][w][lane] = s1;
        part[1][w][lane] = s2;
    }
    __syncthreads();
    if (tid < T.cnt) {
        const size_t pt = (size_t)T.p0 + tid;
        const int m2 = meta2[pt];
        const double mean0 = ((part[0][0][tid] + part[0][1][tid]) + part[0][2][tid]) + part[0][3][tid];
        const double vv = ((part[1][0][tid] + part[1][1][tid]) + part[1][2][tid]) + part[1][3][tid];
        double kss = 0.0;
        for (int q = 0; q < Q; q++) kss += B[(size_t)q * D * D + m2 * D + m2];
        const double var0 = (kss - vv) + hyp[m2];
        double dm = 0.0, extra = 0.0;
        for (int d = 0; d < ncol; d++) dm += (cols.h(pt, m2, d) - Cs[d][tid]) * sm[mean_off_beta(ncol) + d];
        if (mode == MEDGP_MEAN_MARGINAL)
            for (int k = 0; k < ncol; k++) {
                double u = 0.0;
                for (int e = 0; e <= k; e++) u += sm[mean_off_ti(ncol) + (size_t)k * ncol + e] * (cols.h(pt, m2, e) - Cs[e][tid]);
                extra += u * u;
            }
        mean[pt] = mean0 + dm;
        var[pt] = var0 + extra;
    }
}

// the indicator row e_{m2}
struct MeanPostRow {
    __device__ __forceinline__ double h(size_t, int m2, int d) const { return (d == m2) ? 1.0 : 0.0; }
};
// grid = the chunk's tiles
__global__ void __launch_bounds__(256) k_mean_post(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                   const double *__restrict__ work, size_t work_stride, const double *__restrict__ G,
                                                   const double *__restrict__ small, int mode, double *__restrict__ mean,
                                                   double *__restrict__ var) {
    fe_post_body(L, MeanPostRow{}, L.D, tiles, meta2, work, work_stride, G, small, mode, mean, var);
}

