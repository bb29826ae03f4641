// kernels_basis.h -- fixed effects with a general basis, fixed or integrated out (medgp_set_basis, medgp_basis_nlml_grad,
// medgp_basis_posterior_batch).  kernels_mean.h's model y = H beta + f + noise with ANY H (n x p, p <= 64) in place of the indicator
// H[i, d] = [m_i = d]: linear trends, steps and ramps of an intervention, harmonics, dose columns (medgp_amd/basis.py builds them).
// H is resident: medgp_set_basis uploads a slot's rows once, packed in the grouped order (basis_tables.h).  Every formula is
// kernels_mean.h's with p in place of D -- G = L^-1 H, A = Lambda + G^T G, w = z - G b0, c = G^T w, delta = A^-1 c, beta^ = b0 + delta,
// alpha~ = alpha - (P H) beta^, Pm = (P H) chol(A)^-T, W~ = P - Pm Pm^T - alpha~ alpha~^T, the quadratic form as |w - G delta|^2 +
// sum lam_c delta_c^2 -- and the posterior at a point with basis row h*: r = h* - G^T V, mean = V^T z + r^T beta^,
// var = (k** - V^T V + sigma^2) + r^T A^-1 r (FIXED: without the last term).  The definition is tests/basis_truth.py.
//
//   k_basis_g      G = U^T H on fp64 MFMA, one workgroup per 64 rows: G[i, c] = sum_{j <= i} U[j, i] H[j, c], k = j from 0 to the end of
//                  the diagonal block.  Per step of 32 k the 32 x 64 block of U (rows of 64 consecutive doubles: coalesced; masked to
//                  the triangle and to n) and the 32 x 64 block of H (zeros from column p on) are staged in LDS, where the four waves
//                  (16 rows of G each) read both operands; zeros on the padding rows and on the columns >= p
//   k_basis_small  k_mean_small's program (kernels_mean.h: fe_small_body) without the segment table: c and A run over all rows, in
//                  the same fixed orders; the improper entry is the failed pivot of A alone (flat-prior columns that are linearly
//                  dependent on the patient's rows): status -1.  A pivot fails when it is not above basis_pivot_tol(p) = 4 p 2^-52
//                  times the column's own diagonal entry of A: what rounding can leave of an EXACTLY dependent column, whose
//                  pivot is noise of either sign (a plain "pivot <= 0" would pass half of them); a zero column's pivot is 0
//   k_mean_panel, k_mean_wgrad (kernels_mean.h), k_slabsum, k_epilogue, k_pjvp_solve: unchanged.  k_mean_panel takes its column count
//                  from the view's D, so it is handed a view whose D is p; k_mean_wgrad its k range as an argument
//   k_basis_post   k_mean_post's program (fe_post_body) with the tile's rows of h2 (the caller's point order) for e_{m*_j}
// No atomics; every sum in a fixed order over operands of the entry alone (each element of G: k in order within one MFMA chain, no
// split-K): an entry's bits depend neither on its batch-mates, nor on its position, the batch size or the launch chunk (with the
// route pinned, as everywhere); a point's neither on the other points nor on the tile column it lands in.
#pragma once
#include "basis_tables.h"
#include "kernels_mean.h"

// ------------------------------------------------------------------------------------------
// grid = (64-row blocks of the class's largest entry, entries).  Hs: the store; hoff: the offset of every entry's rows in it, in the
// CALLER's entry order.  Wave w owns the rows 16 w .. of the block and the NCT = ceil(p / 16) column tiles below p -- a template
// argument: with the count read at run time (a guard around every MFMA, as k_mean_panel has it) the compiler kept the accumulators
// in 176 VGPRs instead of AGPRs and the kernel ran at 1.6 x k_mean_panel's time.  MFMA operand layout as k_mean_panel:
// lane (li, g) gives A[row li][k g] = U[k g][row li] and B[k g][col li] = H[k g][col li], accumulator element r is C[row 4 r + g][col li].
// ------------------------------------------------------------------------------------------
template <int NCT>
__global__ void __launch_bounds__(256) k_basis_g(MedgpDev L, const double *__restrict__ Hs, const long long *__restrict__ hoff, int p,
                                                 double *__restrict__ G) {
    __shared__ double Us[BASIS_KC][BASIS_LDS_STRIDE], Bs[BASIS_KC][BASIS_LDS_STRIDE];
    const int b = blockIdx.y, I = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, g = lane >> 4;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    if (64 * I >= npad) return;
    const int pos = L.bpos ? L.bpos[b] : b;
    const double *U = L.Linv + (size_t)b * ld * ld;   // U[j][i], j <= i: the upper triangle
    const double *H = Hs + hoff[pos];
    const int i = 64 * I + lane, klast = basis_g_wave_klast(I, w);
    v4d acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (v4d){0.0, 0.0, 0.0, 0.0};
    // wave w stages the rows w, w + 4, ... of a step; the next step's rows are fetched into registers while this step's MFMAs run
    double ur[BASIS_KC / 4], hr[BASIS_KC / 4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < BASIS_KC / 4; s++) {
            const int j = k0 + w + 4 * s;
            ur[s] = (j <= i && i < n) ? U[(size_t)j * ld + i] : 0.0;
            hr[s] = (j < n && lane < p) ? H[basis_h_at(j, p, lane)] : 0.0;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < basis_g_kend(I); k0 += BASIS_KC) {
#pragma unroll
        for (int s = 0; s < BASIS_KC / 4; s++) {
            Us[w + 4 * s][lane] = ur[s];
            Bs[w + 4 * s][lane] = hr[s];
        }
        __syncthreads();
        if (k0 + BASIS_KC < basis_g_kend(I)) fetch(k0 + BASIS_KC);
        if (k0 <= klast)   // wave-uniform: beyond it this wave's rows of U^T are zero
#pragma unroll 2
            for (int kk = 0; kk < BASIS_KC; kk += 4) {
                const double a = Us[kk + g][16 * w + li];
#pragma unroll
                for (int ct = 0; ct < NCT; ct++) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[kk + g][16 * ct + li], acc[ct], 0, 0, 0);
            }
        __syncthreads();
    }
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) G[mean_panel_at(b, ld, 64 * I + 16 * w + 4 * r + g, 16 * ct + li)] = ct < NCT ? acc[ct % NCT][r] : 0.0;
}

// a general column: every row counts, nothing is improper before the algebra; a pivot fails when it is not above
// tol = basis_pivot_tol(p) times the column's own diagonal entry of A (0 for a zero column)
struct BasisSmallCols {
    static constexpr bool IMPROPER = false, SCALED_PIVOT = true;
    double tol;
    __device__ __forceinline__ int row0(int) const { return 0; }
    __device__ __forceinline__ bool improper(int, double) const { return false; }
    __device__ __forceinline__ double pivot_floor(const double *d0, int j) const { return tol * d0[j]; }
};
// grid = the class's entries; in, wvec, small: fe_small_body's with p columns
__global__ void __launch_bounds__(256) k_basis_small(MedgpDev L, const double *__restrict__ G, const double *__restrict__ in, int nbatch_call,
                                                     int mode, int p, double *__restrict__ wvec, double *__restrict__ small) {
    fe_small_body(L, BasisSmallCols{basis_pivot_tol(p)}, p, G, in, nbatch_call, mode, wvec, small);
}

// the point's row of h2: [M][p], the call's point order
struct BasisPostRow {
    const double *h2;
    int p;
    __device__ __forceinline__ double h(size_t pt, int, int d) const { return h2[pt * (size_t)p + d]; }
};
// grid = the chunk's tiles
__global__ void __launch_bounds__(256) k_basis_post(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                    const double *__restrict__ h2, const double *__restrict__ work, size_t work_stride,
                                                    const double *__restrict__ G, const double *__restrict__ small, int mode, int p,
                                                    double *__restrict__ mean, double *__restrict__ var) {
    fe_post_body(L, BasisPostRow{h2, p}, p, tiles, meta2, work, work_stride, G, small, mode, mean, var);
}

