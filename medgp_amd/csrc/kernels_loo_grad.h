// kernels_loo_grad.h -- the negative leave-one-out log pseudo-likelihood and its hyper-parameter gradient (medgp_loo_grad).
// Works behind one pipeline run that left U = L^-T (upper triangle of Linv) and alpha = K^-1 y of every entry.  With
//   P = K^-1 = U U^T,  d_i = P_ii,  u_i = alpha_i / d_i,  s_i = (1 + alpha_i^2 / d_i) / d_i,  v = P u,
//   log p(y_i | y_-i) = 1/2 log d_i - 1/2 alpha_i^2 / d_i - 1/2 log 2 pi              (Rasmussen & Williams 5.4.2)
// the objective is J = - sum_i log p(y_i | y_-i) and its gradient (from R&W eq. 5.13)
//   dJ / d theta_h = 1/2 tr(W_loo dK / d theta_h),     W_loo = P diag(s) P - (alpha v^T + v alpha^T):
// the shape of the marginal-likelihood gradient with W_loo in the place of W = K^-1 - alpha alpha^T, so everything behind the W
// tile (block sums, wdiag, k_slabsum, k_epilogue) is the nlml gradient's.  The reference has no such output: the definition is
// tests/loo_grad_truth.py.
//   k_loo_kinv     one workgroup per lower 64 x 64 tile: P = U U^T on fp64 MFMA (wg_phase1, masked), stored as a FULL symmetric
//                  matrix into the entry's Kmat block (dead behind the factorisation), identity on the padding
//   k_loo_vec      pass 0: d (from the rows of U, the very sum of k_loo_diag), u, s and log p of a 16-row block;
//                  pass 1: v = P u of a 16-row block, and (block 0) J = - sum_i log p_i in a fixed order -> scal[2]
//   k_loo_wgrad    one workgroup per lower tile: G = sum_k P[i,k] s_k P[j,k] over ALL k (no triangular structure), the tile
//                  G - alpha_i v_j - v_i alpha_j, then k_wgrad's phases 2 and 3 (slab pieces written once, wdiag exported)
// No atomics, every sum in a fixed order over operands of the entry alone: an entry's bits do not depend on its batch-mates.
// The per-entry vectors live in a buffer of the call: [u | s | v | log p], 4 ld doubles per entry.
// k_loo_kinv and k_loo_wgrad are built from the pieces of kernels_wgrad.h (prologue, wg_phase1 / 2 / 3); only the hooks and the tile
// element below are their own.
#pragma once
#include "kernels_wgrad.h"

// two adjacent elements of row `row` of U starting at column `col`: what lies left of the diagonal is a leftover of the factorisation
__device__ __forceinline__ v2d loo_mask_u(v2d x, int col, int row) {
    x[0] = (col >= row) ? x[0] : 0.0;
    x[1] = (col + 1 >= row) ? x[1] : 0.0;
    return x;
}

// phase-1 hook of k_loo_kinv: only the first two chunks touch a diagonal block of U; both operands are masked there
struct LooMaskHook {
    __device__ __forceinline__ v2d staged(v2d x, int c, int row, int col) const { return c < 2 ? loo_mask_u(x, col, row) : x; }
    __device__ __forceinline__ v2d streamed(v2d x, int c, int row, int col) const { return c < 2 ? loo_mask_u(x, col, row) : x; }
};
// phase-1 hook of k_loo_wgrad: the staged J rows are multiplied by s_k on their way into LDS
struct LooScaleHook {
    const double *s;
    __device__ __forceinline__ v2d staged(v2d x, int, int, int col) const { return x * *(const v2d *)(s + col); }
    __device__ __forceinline__ v2d streamed(v2d x, int, int, int) const { return x; }
};
// phase-3 element of k_loo_wgrad: G_ij - alpha_i v_j - v_i alpha_j; the row and column constants carry v beside alpha
struct LooElem {
    static constexpr int NX = 1;
    const double *v;
    __device__ __forceinline__ double extra(int k) const { return v[k]; }
    __device__ __forceinline__ double elem(double ws, double ai, double aj, double vi, double vj) const { return (ws - ai * vj) - vi * aj; }
};

// ------------------------------------------------------------------------------------------
// P tile (I, J), I >= J: sum over the columns k >= 64 I of U[I rows][k] U[J rows][k]: k_wgrad's prologue and phases 1 and 2 with the
// mask hook.  The tile leaves through LDS so that both it and its mirror image are stored as contiguous rows.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG_THREADS) k_loo_kinv(MedgpDev L, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    double (*Ws)[66] = (double (*)[66])smem;   // Ws[64][66]
    WG_PROLOGUE(false);
    const int n = T.n, ld = T.ld, I = T.I, J = T.J;
    const double *U = L.Linv + (size_t)T.b * ld * ld;
    double *P = L.Kmat + (size_t)T.b * ld * ld;

    const WgAcc acc = wg_phase1<false>(smem, T, U, 64 * I, LooMaskHook());   // (the masked U would allow the skip of zero stretches; not taken up here)
    wg_phase2(acc, smem, T);   // diagonal tile: the column strips right of a wave's rows come from the mirror image
    for (int x = T.tid; x < 64 * 64; x += WG_THREADS) {
        const int r = x >> 6, cc = x & 63;
        {   // row r of the tile
            const int gi = 64 * I + r, gj = 64 * J + cc;
            const double val = (I == J && cc > r) ? Ws[cc][r] : Ws[r][cc];
            P[(size_t)gi * ld + gj] = (gi < n && gj < n) ? val : (gi == gj ? 1.0 : 0.0);
        }
        if (I != J) {   // row r of its mirror image
            const int gi = 64 * J + r, gj = 64 * I + cc;
            P[(size_t)gi * ld + gj] = (gi < n && gj < n) ? Ws[cc][r] : 0.0;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The vectors of an entry; vec = [u | s | v | log p] of the class view, 4 ld doubles per entry.  grid = (16-row blocks, entries),
// wave w of a workgroup owns 4 rows at once (four independent load streams), the lanes stride over the rows' columns and add their
// 64 partial sums by a butterfly.
//   mode 0: d_i = sum_{k >= i} U[i][k]^2 exactly as k_loo_diag forms it, u, s, log p_i; zeros on the padding rows [n, npad)
//   mode 1: v_i = sum_k P[i][k] u_k over [0, n); zeros on the padding; block 0 also adds up J
//   mode 2: (objective only, one block per entry) J alone
// (One workgroup per entry, rows in turn, left a single N = 2048 patient on one CU: 0.30 ms for both passes.)
// J = - sum_i log p_i: thread t adds the observations t, t + 256, ..., the 256 sums go through one tree.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_loo_vec(MedgpDev L, double *__restrict__ vec, int mode, double log2pi) {
    __shared__ double red[256];
    const int b = blockIdx.y, rb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    if (16 * rb >= npad) return;
    double *uv = vec + (size_t)b * 4 * ld, *sv = uv + ld, *vv = sv + ld, *lp = vv + ld;
    const int r0 = 16 * rb + 4 * w;   // this wave's four rows (one 64-block: they share the first column of their sums)
    if (mode == 0) {
        const double *U = L.Linv + (size_t)b * ld * ld + (size_t)r0 * ld, *al = L.alpha + (size_t)b * ld;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = (r0 & ~63) + lane; k < n; k += 64) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const double u = (k >= r0 + e) ? U[(size_t)e * ld + k] : 0.0;
                s[e] += u * u;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
            for (int off = 32; off > 0; off >>= 1) s[e] += __shfl_xor(s[e], off);
        if (lane < 4) {
            const int i = r0 + lane;
            const double d = lane == 0 ? s[0] : (lane == 1 ? s[1] : (lane == 2 ? s[2] : s[3]));
            if (i < n) {
                const double a = al[i], q = a * a / d;
                uv[i] = a / d;
                sv[i] = (1.0 + q) / d;
                lp[i] = -0.5 * q + 0.5 * log(d) - 0.5 * log2pi;
            } else {
                uv[i] = 0.0; sv[i] = 0.0; lp[i] = 0.0;
            }
        }
        return;
    }
    if (mode == 1) {
        const double *P = L.Kmat + (size_t)b * ld * ld + (size_t)r0 * ld;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = lane; k < n; k += 64) {
            const double u = uv[k];
#pragma unroll
            for (int e = 0; e < 4; e++) s[e] += P[(size_t)e * ld + k] * u;
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
            for (int off = 32; off > 0; off >>= 1) s[e] += __shfl_xor(s[e], off);
        if (lane < 4) {
            const int i = r0 + lane;
            const double v = lane == 0 ? s[0] : (lane == 1 ? s[1] : (lane == 2 ? s[2] : s[3]));
            vv[i] = (i < n) ? v : 0.0;
        }
    }
    if (rb != 0) return;
    double a = 0.0;
    for (int i = tid; i < n; i += 256) a += lp[i];
    red[tid] = a;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) L.scal[b * 4 + 2] = -red[0];
}

// ------------------------------------------------------------------------------------------
// W_loo tile + gradient block reductions: k_wgrad's prologue and phases (kernels_wgrad.h), with
//   phase 1  both operands rows of the full symmetric P, the contraction over all of [0, npad), and the staged J rows
//            multiplied by s_k on their way into LDS (s = 0 on the padding: its identity adds nothing)
//   phase 3  the tile element  G_ij - alpha_i v_j - v_i alpha_j
// QT / Q0 as in k_wgrad: 8 < Q <= 16 takes two launches, each forming G again.
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, WG_MINWAVES) k_loo_wgrad(MedgpDev L, const double *__restrict__ vec, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<LooElem, QT>];
    WG_PROLOGUE(false);
    const double *P = L.Kmat + (size_t)T.b * T.ld * T.ld;
    const double *svec = vec + (size_t)T.b * 4 * T.ld + T.ld, *vvec = svec + T.ld;

    const WgAcc acc = wg_phase1<false>(smem, T, P, 0, LooScaleHook{svec});   // G = P diag(s) P: full rows from column 0, no zero stretches
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, LooElem{vvec});
}
