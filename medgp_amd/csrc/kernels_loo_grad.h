// kernels_loo_grad.h -- the negative leave-one-out log pseudo-likelihood and its hyper-parameter gradient (medgp_loo_grad).
// Works behind one pipeline run that left U = L^-T (upper triangle of Linv) and alpha = K^-1 y of every entry.  With
//   P = K^-1 = U U^T,  d_i = P_ii,  u_i = alpha_i / d_i,  s_i = (1 + alpha_i^2 / d_i) / d_i,  v = P u,
//   log p(y_i | y_-i) = 1/2 log d_i - 1/2 alpha_i^2 / d_i - 1/2 log 2 pi              (Rasmussen & Williams 5.4.2)
// the objective is J = - sum_i log p(y_i | y_-i) and its gradient (from R&W eq. 5.13)
//   dJ / d theta_h = 1/2 tr(W_loo dK / d theta_h),     W_loo = P diag(s) P - (alpha v^T + v alpha^T):
// the shape of the marginal-likelihood gradient with W_loo in the place of W = K^-1 - alpha alpha^T, so everything behind the W
// tile (block sums, wdiag, k_slabsum, k_epilogue) is the nlml gradient's.  The reference has no such output: the definition is
// tests/loo_grad_truth.py.
//   k_loo_kinv     one workgroup per lower 64 x 64 tile: P = U U^T on fp64 MFMA (k_wgrad's phase 1), stored as a FULL symmetric
//                  matrix into the entry's Kmat block (dead behind the factorisation), identity on the padding
//   k_loo_vec      pass 0: d (from the rows of U, the very sum of k_loo_diag), u, s and log p of a 16-row block;
//                  pass 1: v = P u of a 16-row block, and (block 0) J = - sum_i log p_i in a fixed order -> scal[2]
//   k_loo_wgrad    one workgroup per lower tile: G = sum_k P[i,k] s_k P[j,k] over ALL k (no triangular structure), the tile
//                  G - alpha_i v_j - v_i alpha_j, then k_wgrad's phases 2 and 3 (slab pieces written once, wdiag exported)
// No atomics, every sum in a fixed order over operands of the entry alone: an entry's bits do not depend on its batch-mates.
// The per-entry vectors live in a buffer of the call: [u | s | v | log p], 4 ld doubles per entry.
#pragma once
#include "kernels_wgrad.h"

// workgroup id -> (entry, tile) as k_wgrad deals them: an entry's tiles share an XCD (and its L2) from 64 entries on, and are
// spread over all XCDs below that (stride nbp of the entry index: nbatch, or nbatch | 1 for a ragged class)
__device__ __forceinline__ bool loo_tile_of(int x, int nbatch, int ntiles, int nbp, int &b, int &tix) {
    if (nbatch >= 64) {
        const int xcd = x & 7, rest = x >> 3;
        b = (rest / ntiles) * 8 + xcd;
        tix = rest % ntiles;
    } else {
        if (x >= nbp * ntiles) return false;
        b = x % nbp;
        tix = x / nbp;
    }
    return b < nbatch;
}

// two adjacent elements of row `row` of U starting at column `col`: what lies left of the diagonal is a leftover of the factorisation
__device__ __forceinline__ v2d loo_mask_u(v2d x, int col, int row) {
    x[0] = (col >= row) ? x[0] : 0.0;
    x[1] = (col + 1 >= row) ? x[1] : 0.0;
    return x;
}

// ------------------------------------------------------------------------------------------
// P tile (I, J), I >= J: sum over the columns k >= 64 I of U[I rows][k] U[J rows][k].  The J rows are staged through LDS, the I
// rows streamed (k_wgrad's phase 1, one chunk of WG_KC columns ahead).  Only the first two chunks touch a diagonal block of U;
// they are masked.  The tile leaves through LDS so that both it and its mirror image are stored as contiguous rows.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG_THREADS) k_loo_kinv(MedgpDev L, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[2 * 64 * (WG_KC + 2)];
    typedef double (*BsT)[64][WG_KC + 2];
    BsT Bs = (BsT)smem;                       // Bs[2][64][34]
    double (*Ws)[66] = (double (*)[66])smem;   // Ws[64][66]
    int b, tix;
    if (!loo_tile_of(blockIdx.x, nbatch, ntiles, nbp, b, tix)) return;
    if (L.status[b] < 0) return;
    const int slot = __builtin_amdgcn_readfirstlane(L.bslot[b]);
    const int n = __builtin_amdgcn_readfirstlane(L.pn[slot]);
    const int ld = L.ldn, npad = medgp_roundup(n, 64), nb = npad / 64;
    int I, J;
    tile_decode(tix, I, J);
    if (I >= nb) return;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *U = L.Linv + (size_t)b * ld * ld;
    double *P = L.Kmat + (size_t)b * ld * ld;

    v4d acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[ct] = (v4d){0.0, 0.0, 0.0, 0.0};
    {
        const int k0 = 64 * I, nch = (npad - k0) / WG_KC;
        const int ctmax = (I == J) ? w : 3;   // diagonal tile: the column strips right of this wave's rows come from the mirror image
        const int arow = 64 * I + 16 * w + li, srow = tid >> 2, scg = (tid & 3) * 8, brow = 64 * J + srow;
        const double *Arow = U + (size_t)arow * ld + k0 + 2 * g;
        const double *Bsrc = U + (size_t)brow * ld + k0 + scg;
        v2d bst[4], an[4];
#pragma unroll
        for (int u = 0; u < 4; u++) bst[u] = loo_mask_u(*(const v2d *)(Bsrc + 2 * u), k0 + scg + 2 * u, brow);
#pragma unroll
        for (int h = 0; h < 4; h++) an[h] = loo_mask_u(*(const v2d *)(Arow + 8 * h), k0 + 2 * g + 8 * h, arow);
#pragma unroll
        for (int u = 0; u < 4; u++) *(v2d *)&Bs[0][srow][scg + 2 * u] = bst[u];
        __syncthreads();
        for (int c = 0; c < nch; c++) {
            const int buf = c & 1;
            v2d ac[4];
#pragma unroll
            for (int h = 0; h < 4; h++) ac[h] = an[h];
            if (c + 1 < nch) {
                const int kc = k0 + (c + 1) * WG_KC;
#pragma unroll
                for (int u = 0; u < 4; u++) bst[u] = *(const v2d *)(Bsrc + (c + 1) * WG_KC + 2 * u);
#pragma unroll
                for (int h = 0; h < 4; h++) an[h] = *(const v2d *)(Arow + (c + 1) * WG_KC + 8 * h);
                if (c == 0) {   // the second half of the diagonal block
#pragma unroll
                    for (int u = 0; u < 4; u++) bst[u] = loo_mask_u(bst[u], kc + scg + 2 * u, brow);
#pragma unroll
                    for (int h = 0; h < 4; h++) an[h] = loo_mask_u(an[h], kc + 2 * g + 8 * h, arow);
                }
            }
            WG_CHUNK_MFMA(ac, buf);
            if (c + 1 < nch) {
#pragma unroll
                for (int u = 0; u < 4; u++) *(v2d *)&Bs[buf ^ 1][srow][scg + 2 * u] = bst[u];
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) Ws[16 * w + 4 * r + g][16 * ct + li] = acc[ct][r];
    __syncthreads();
    for (int x = tid; x < 64 * 64; x += WG_THREADS) {
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
// W_loo tile + gradient block reductions.  Geometry, workgroup mapping, phases 2 and 3 are k_wgrad's (kernels_wgrad.h, which this
// kernel restates so that the nlml gradient's kernel stays as it was measured); what differs:
//   phase 1  both operands are rows of the full symmetric P, the contraction runs over all of [0, npad), and the staged J rows
//            are multiplied by s_k on their way into LDS (s = 0 on the padding: its identity adds nothing)
//   phase 3  the tile element is  G_ij - alpha_i v_j - v_i alpha_j  (the row constants carry v_i beside alpha_i)
// QT / Q0 as in k_wgrad: 8 < Q <= 16 takes two launches, each forming G again.
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, WG_MINWAVES) k_loo_wgrad(MedgpDev L, const double *__restrict__ vec, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[2 * 64 * (WG_KC + 2)];
    typedef double (*BsT)[64][WG_KC + 2];
    BsT Bs = (BsT)smem;                       // Bs[2][64][34]
    double (*Ws)[66] = (double (*)[66])smem;   // Ws[64][66]
    __shared__ __attribute__((aligned(16))) double rowc[4][16][4 + 2 * QT];   // row constants of each wave's 16 rows: t, alpha, v, -, (cos, sin) x QT

    int b, tix;
    if (!loo_tile_of(blockIdx.x, nbatch, ntiles, nbp, b, tix)) return;
    if (L.status[b] < 0) return;
    const int slot = __builtin_amdgcn_readfirstlane(L.bslot[b]);
    const int n = __builtin_amdgcn_readfirstlane(L.pn[slot]);
    const int ld = L.ldn, npad = medgp_roundup(n, 64), nb = npad / 64;
    int I, J;
    tile_decode(tix, I, J);
    if (I >= nb) return;
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *P = L.Kmat + (size_t)b * ld * ld;
    const double *svec = vec + (size_t)b * 4 * ld + ld, *vvec = svec + ld;

    // ---------------- phase 1: acc[ct] (rows 16w.. of block I, cols 16ct.. of block J) of G = P diag(s) P
    v4d acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[ct] = (v4d){0.0, 0.0, 0.0, 0.0};
    {
        const int nch = npad / WG_KC;
        const int ctmax = (I == J) ? w : 3;   // wave-uniform
        const double *Arow = P + (size_t)(64 * I + 16 * w + li) * ld + 2 * g;
        const int srow = tid >> 2, scg = (tid & 3) * 8;
        const double *Bsrc = P + (size_t)(64 * J + srow) * ld + scg;
        const double *Ssrc = svec + scg;
        v2d bst[4], an[4];
#pragma unroll
        for (int u = 0; u < 4; u++) bst[u] = *(const v2d *)(Bsrc + 2 * u) * *(const v2d *)(Ssrc + 2 * u);
#pragma unroll
        for (int h = 0; h < 4; h++) an[h] = *(const v2d *)(Arow + 8 * h);
#pragma unroll
        for (int u = 0; u < 4; u++) *(v2d *)&Bs[0][srow][scg + 2 * u] = bst[u];
        __syncthreads();
        for (int c = 0; c < nch; c++) {
            const int buf = c & 1;
            v2d ac[4];
#pragma unroll
            for (int h = 0; h < 4; h++) ac[h] = an[h];
            if (c + 1 < nch) {
#pragma unroll
                for (int u = 0; u < 4; u++) bst[u] = *(const v2d *)(Bsrc + (c + 1) * WG_KC + 2 * u) * *(const v2d *)(Ssrc + (c + 1) * WG_KC + 2 * u);
#pragma unroll
                for (int h = 0; h < 4; h++) an[h] = *(const v2d *)(Arow + (c + 1) * WG_KC + 8 * h);
            }
            WG_CHUNK_MFMA(ac, buf);
            if (c + 1 < nch) {
#pragma unroll
                for (int u = 0; u < 4; u++) *(v2d *)&Bs[buf ^ 1][srow][scg + 2 * u] = bst[u];
            }
            __syncthreads();
        }
    }
    // ---------------- phase 2: G tile -> LDS (all waves are past the last staging read: barrier above)
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) Ws[16 * w + 4 * r + g][16 * ct + li] = acc[ct][r];
    __syncthreads();

    // ---------------- phase 3 (k_wgrad's, on the element G_ij - alpha_i v_j - v_i alpha_j)
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *t = L.pt + (size_t)slot * L.pld;
    const int *meta = L.pmeta + (size_t)slot * L.pld;
    const double *alpha = L.alpha + (size_t)b * ld;
    const int *seg = L.pseg + (size_t)slot * (L.D + 1);
    const int *roff = L.proff + (size_t)slot * (L.D + 1), *coff = L.pcoff + (size_t)slot * (L.D + 1);
    const double *csb = L.cs + ((size_t)b * L.Q + Q0) * ld, *snb = L.sn + ((size_t)b * L.Q + Q0) * ld;
    double *slab = L.slab + (size_t)b * L.slab_stride;
    const int Qall = L.Q;   // the slab planes are [S | SM | SV] x ALL components
    const int Rmax = L.slab_R, Cmax = L.slab_C;

    double wq[QT], cq[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) { wq[q] = hyp[hyp_off_w(L) + Q0 + q]; cq[q] = hyp[hyp_off_c(L) + Q0 + q]; }
    double cq2n[QT];   // -c_q log2(e): exp(-c_q dt^2) = 2^(cq2n dt^2), as in k_assemble_t
#pragma unroll
    for (int q = 0; q < QT; q++) cq2n[q] = uniform_d(-cq[q] * MEDGP_LOG2E);
    // column constants of this lane
    const int j = 64 * J + lane;
    const bool jv = j < n;
    const double tj = t[j], aj = alpha[j], vj = vvec[j];
    const int mj = jv ? meta[j] : -1;
    double csj[QT], snj[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) { csj[q] = csb[q * ld + j]; snj[q] = snb[q * ld + j]; }
    // column segments inside the tile: leader lanes and their segment ends
    const int mprev = __shfl_up(mj, 1);
    const bool leader = (lane == 0) || (mj != mprev);
    const unsigned long long lmask = __ballot(leader);
    int segend;
    {
        unsigned long long above = (lane == 63) ? 0ull : (lmask >> (lane + 1));
        segend = above ? (lane + 1 + __builtin_ctzll(above)) : 64;
    }
    // first lane of this lane's column segment, and whether this lane is its last one (it writes the segment sum)
    const unsigned long long upto = lmask & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
    const int segstart = 63 - __builtin_clzll(upto);
    const bool seglast = (lane == segend - 1);
    const int cslot = (mj >= 0) ? coff[mj] + (J - seg[mj] / 64) : 0;
    const int rg = 4 * I + w;   // global 16-row group of this wave

    double sS[QT], sM[QT], sV[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) { sS[q] = 0.0; sM[q] = 0.0; sV[q] = 0.0; }
    int mcur = -2;
    // row constants of the wave's 16 rows (lane r holds row r, lanes >= 16 mirror), handed round through LDS broadcasts
    const int irow = 64 * I + 16 * w + (lane & 15);
    const double r_t = t[irow], r_a = alpha[irow], r_v = vvec[irow];
    const int r_m = (irow < n) ? meta[irow] : -1;
    if (lane < 16) {
        rowc[w][lane][0] = r_t; rowc[w][lane][1] = r_a; rowc[w][lane][2] = r_v; rowc[w][lane][3] = 0.0;
#pragma unroll
        for (int q = 0; q < QT; q++) { rowc[w][lane][4 + 2 * q] = csb[q * ld + irow]; rowc[w][lane][5 + 2 * q] = snb[q * ld + irow]; }
    }
    __builtin_amdgcn_wave_barrier();
    for (int rr = 0; rr <= 16; rr++) {
        const int i = 64 * I + 16 * w + rr;
        int mi = -1;
        if (rr < 16) mi = __builtin_amdgcn_readlane(r_m, rr);          // wave-uniform
        if (mi != mcur) {
            // flush the running sums of row output mcur (skip padding / initial state)
            if (mcur >= 0) {
                const int rslot = roff[mcur] + (rg - seg[mcur] / 16);
                // segmented inclusive scan over the lanes (6 shuffle steps, fixed order): the last lane of every column
                // segment ends up with the segment sum
                double fv[3 * QT];
#pragma unroll
                for (int q = 0; q < QT; q++) { fv[q] = sS[q]; fv[QT + q] = -wq[q] * sM[q]; fv[2 * QT + q] = -2.0 * cq[q] * sV[q]; }
#pragma unroll
                for (int dlt = 1; dlt < 64; dlt <<= 1) {
                    double up[3 * QT];
#pragma unroll
                    for (int k = 0; k < 3 * QT; k++) up[k] = __shfl_up(fv[k], dlt);
                    if (lane - dlt >= segstart) {
#pragma unroll
                        for (int k = 0; k < 3 * QT; k++) fv[k] += up[k];
                    }
                }
                if (seglast && mj >= 0) {
#pragma unroll
                    for (int k = 0; k < 3 * QT; k++) slab[((size_t)((k / QT) * Qall + Q0 + (k % QT)) * Rmax + rslot) * Cmax + cslot] = fv[k];
                }
            }
#pragma unroll
            for (int q = 0; q < QT; q++) { sS[q] = 0.0; sM[q] = 0.0; sV[q] = 0.0; }
            mcur = mi;
        }
        if (rr == 16 || mi < 0) continue;
        const v2d ta = *(const v2d *)&rowc[w][rr][0];
        const double ti = ta[0], ai = ta[1], vi = rowc[w][rr][2];
        double wv = (Ws[16 * w + rr][lane] - ai * vj) - vi * aj;
        if (I == J && j == i) L.wdiag[(size_t)b * ld + i] = wv;   // noise gradient needs diag(W_loo)
        const bool valid = jv && (j <= i);
        wv = valid ? ((mi == mj && j < i) ? 2.0 * wv : wv) : 0.0;
        const double dt = ti - tj, dd = dt * dt;
#pragma unroll
        for (int q = 0; q < QT; q++) {
            const v2d csn = *(const v2d *)&rowc[w][rr][4 + 2 * q];
            const double ci = csn[0], si = csn[1];
            const double we = wv * exp2_nonpos(cq2n[q] * dd);
            const double cd = ci * csj[q] + si * snj[q];
            const double sd = si * csj[q] - ci * snj[q];
            const double p = we * cd;
            sS[q] += p;
            sM[q] += (we * sd) * dt;
            sV[q] += p * dd;
        }
    }
}
