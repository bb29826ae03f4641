// kernels_lgo_grad.h -- the negative leave-group-out log pseudo-likelihood and its hyper-parameter gradient (medgp_lgo_grad).
// Works behind one pipeline run that left U = L^-T (upper triangle of Linv) and alpha = K^-1 y of every entry.  With P = K^-1 and, for
// every non-empty group g >= 0 with the ascending index list B_g,
//   M_g = P[B_g, B_g] = R R^T,   w = R^-1 alpha_B,   r_g = M_g^-1 alpha_B = R^-T w,
//   lpd_g = -1/2 w^T w + sum_j log R_jj - |B_g| / 2 log 2 pi                      (medgp_loo_batch's lpd, formed by its kernels)
//   J = - sum_g lpd_g,     S = sum_g E_g (M_g^-1 + r_g r_g^T) E_g^T,     r = sum_g E_g r_g,     v = P r,
//   dJ / d theta_h = 1/2 tr(W_lgo dK / d theta_h),     W_lgo = P S P - (alpha v^T + v alpha^T):
// the shape of the marginal-likelihood gradient with W_lgo in the place of W, so everything behind the W tile (block sums, wdiag,
// k_slabsum, k_epilogue) is the nlml gradient's.  A singleton group is the scalar case: M = d_i, r = u_i, S = s_i of kernels_loo_grad.h,
// and its numbers ARE k_loo_vec's (mode 0).  The reference has no such output: the definition is tests/lgo_grad_truth.py.
//   k_lgo_mask    behind k_loo_vec mode 0 (u, s, log p of EVERY row): rows that are no singleton group get u = s = 0, the log p of a
//                 singleton goes to its group's lpd.  The u slot of the entry's vectors is r from here on.
//   k_lgo_prep    Tt = P diag(s): the singleton columns of Tt = P S, zeros in every other column (id -1, padding; the columns of larger
//                 groups are written by k_lgo_t afterwards)
//   k_lgo_inv     behind k_loo_gram / k_postfactor / k_loo_solve (R in the group's first block, w behind the second): one workgroup per
//                 64-column tile of X = R^-1: loo_block_column_inverse (kernels_loo.h), the function k_loo_solve's column job calls,
//                 here with every block row stored and no variances
//   k_lgo_s       one workgroup per (group, lower tile pair I >= J): S_g = X^T X + r_g r_g^T on fp64 MFMA, the contraction from block row
//                 I on (X is lower triangular); r_g = X^T w in fp64, scattered to the entry's r by the diagonal tiles.  S_g is stored as a
//                 full symmetric block over R (dead behind k_lgo_inv and the vector solves).
//   k_lgo_t       one workgroup per (group, 64-row block of P): Tt[rows, B_g] = P[rows, B_g] S_g on fp64 MFMA.  P is symmetric: the
//                 gathered operand P[i, B_g[k]] is read as P[B_g[k], i], contiguous in i.  The rows of S_g go through LDS.
//   k_lgo_obj     J = - sum_g lpd_g over the entry's non-empty groups in the order of their first members, one thread -> scal[2]
//   k_lgo_wgrad   one workgroup per lower tile (I, J): G = sum_k P[i,k] Tt[j,k] over all of [0, npad) (fc_phase1, two operand matrices),
//                 the tile G - alpha_i v_j - v_i alpha_j, then k_wgrad's phases 2 and 3 with the LOO tile element
// v = P r is k_loo_vec mode 1 with r in the u slot (its J is overwritten by k_lgo_obj).
// No atomics, every sum in a fixed order over operands of the entry (of the group) alone: an entry's bits do not depend on its
// batch-mates, on the labels of its groups or on the launch chunk.
// The block of a group (inference_tables.h): [mpad x mpad] R -> S_g | [mpad x mpad] X | [mpad] w | [mpad] -.
#pragma once
#include "kernels_loo.h"
#include "kernels_loo_grad.h"
#include "kernels_forecast_grad.h"

// sgl: per row of every entry (laid out like the vectors: ld ints per entry) the group of the call a singleton row is, or -1
__global__ void __launch_bounds__(256) k_lgo_mask(MedgpDev L, double *__restrict__ vec, const int *__restrict__ sgl, double *__restrict__ lpd) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    if (i >= npad) return;
    double *uv = vec + (size_t)b * 4 * ld, *sv = uv + ld, *lp = sv + 2 * (size_t)ld;
    const int g = sgl[(size_t)b * ld + i];
    if (g < 0) { uv[i] = 0.0; sv[i] = 0.0; }
    else lpd[g] = lp[i];
}

// grid = (column blocks, 4-row groups, entries); P = the entry's Kmat block behind k_loo_kinv, Tm laid out like Kmat
__global__ void __launch_bounds__(256) k_lgo_prep(MedgpDev L, const double *__restrict__ vec, double *__restrict__ Tm) {
    const int b = blockIdx.z;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const int i = 64 * blockIdx.x + (threadIdx.x & 63), j = 4 * blockIdx.y + (threadIdx.x >> 6);
    if (i >= npad || j >= npad) return;
    const double *sv = vec + (size_t)b * 4 * ld + ld;
    const size_t at = (size_t)b * ld * ld + (size_t)j * ld + i;
    Tm[at] = L.Kmat[at] * sv[i];   // (s = 0 on every row that is no singleton group)
}

// X = R^-1, columns 64 c .. 64 c + 63 (job.I = c): loo_block_column_inverse (kernels_loo.h) with every block row stored and nothing
// summed.  X has exact zeros above the diagonal of its diagonal blocks and the identity on the padding; the blocks above the diagonal
// are never written and never read.
__global__ void __launch_bounds__(256) k_lgo_inv(MedgpDev L, const JointPat *__restrict__ groups, const JointTile *__restrict__ jobs,
                                                 double *__restrict__ Mbuf, const int *__restrict__ gstat) {
    __shared__ LooSolveSmem sm;
    const JointTile T = jobs[blockIdx.x];
    const JointPat P = groups[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, mpad = medgp_roundup(P.m, 64);
    if (L.status[b] < 0 || gstat[P.b] < 0) return;
    const double *R = Mbuf + P.coff;
    loo_block_column_inverse<true, false>(sm, R, Mbuf + P.coff + (size_t)mpad * mpad, mpad, T.I, tid, w, li, g);
}

// ------------------------------------------------------------------------------------------
// S_IJ = sum_{k >= 64 I} X[k][I cols]^T X[k][J cols] + r_I r_J^T for the tile pair (I, J), I >= J, of a group.  Both operands are rows of
// X: those of the J columns are staged through LDS POST_KC rows at a time, those of the I columns read from memory (16 adjacent doubles per
// quarter wave).  r_I and r_J (128 columns, one thread each, rows in order: the same bits in every tile) first.  The tile and, off the
// diagonal, its mirror image go to the group's first block.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lgo_s(MedgpDev L, const JointPat *__restrict__ groups, const JointTile *__restrict__ pairs,
                                               const LooRow *__restrict__ rows, double *__restrict__ Mbuf, const int *__restrict__ gstat,
                                               double *__restrict__ vec) {
    __shared__ double Vs[POST_KC * POST_LS];
    __shared__ double rs[128];
    const JointTile T = pairs[blockIdx.x];
    const JointPat P = groups[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, m = P.m, mpad = medgp_roundup(m, 64), I = T.I, J = T.J;
    if (L.status[b] < 0 || gstat[P.b] < 0) return;
    double *Sg = Mbuf + P.coff;
    const double *X = Sg + (size_t)mpad * mpad, *wv = X + (size_t)mpad * mpad;
    if (tid < 128) {
        const int blk = tid < 64 ? I : J, col = 64 * blk + (tid & 63);
        double s = 0.0;
        for (int k = 64 * blk; k < mpad; k++) s += X[(size_t)k * mpad + col] * wv[k];
        rs[tid] = s;
    }
    v4d acc[4];
#pragma unroll
    for (int cs = 0; cs < 4; cs++) acc[cs] = v4d{0.0, 0.0, 0.0, 0.0};
    const double *Xa = X + 64 * I + 16 * w + li;
    panel_product<0>(acc, Vs, 64 * I, mpad, li, g,   // (its first barrier: rs is written)
                     [&](int kk) { panel_stage_rows(Vs, X + 64 * J, kk, mpad, tid); }, [&](int k) { return Xa[(size_t)k * mpad]; });
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int ti = 16 * w + 4 * r + g;
#pragma unroll
        for (int cs = 0; cs < 4; cs++) {
            const int tj = 16 * cs + li;
            const double val = acc[cs][r] + rs[ti] * rs[64 + tj];
            Sg[(size_t)(64 * I + ti) * mpad + 64 * J + tj] = val;
            if (I != J) Sg[(size_t)(64 * J + tj) * mpad + 64 * I + ti] = val;
        }
    }
    if (I == J && tid < 64 && 64 * I + tid < m) vec[(size_t)b * 4 * L.ldn + rows[P.p0 + 64 * I + tid].r] = rs[tid];
}

// ------------------------------------------------------------------------------------------
// Tt[64 rb + i][B[p]] = sum_{k < m} P[B[k]][64 rb + i] S_g[k][p] for row block rb (job.I) of the entry and every column p of the group,
// 64 columns at a time.  Wave w owns the rows 16 w .. 16 w + 15 and all four 16-column strips; the rows k of S_g are staged through LDS
// (POST_KC x POST_LS, row-major: no transposed store).  Rows and columns of the group's padding are masked (S_g holds the identity there).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lgo_t(MedgpDev L, const JointPat *__restrict__ groups, const JointTile *__restrict__ jobs,
                                               const LooRow *__restrict__ rows, const double *__restrict__ Mbuf, const int *__restrict__ gstat,
                                               double *__restrict__ Tm) {
    __shared__ double Vs[POST_KC * POST_LS];
    const JointTile T = jobs[blockIdx.x];
    const JointPat P = groups[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, m = P.m, mpad = medgp_roundup(m, 64), nt = mpad / 64, rb = T.I;
    if (L.status[b] < 0 || gstat[P.b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    if (64 * rb >= npad) return;
    const double *Sg = Mbuf + P.coff;
    const double *Pm = L.Kmat + (size_t)b * ld * ld + 64 * rb + 16 * w + li;
    double *Tb = Tm + (size_t)b * ld * ld;
    const LooRow *rw = rows + P.p0;
    for (int J = 0; J < nt; J++) {
        v4d acc[4];
#pragma unroll
        for (int cs = 0; cs < 4; cs++) acc[cs] = v4d{0.0, 0.0, 0.0, 0.0};
        panel_product<0>(acc, Vs, 0, mpad, li, g, [&](int kk) { panel_stage_rows(Vs, Sg + 64 * J, kk, mpad, tid); },
                         [&](int k) { return k < m ? Pm[(size_t)rw[k].r * ld] : 0.0; });
#pragma unroll
        for (int cs = 0; cs < 4; cs++) {
            const int p = 64 * J + 16 * cs + li;
            if (p >= m) continue;
            const int col = rw[p].r;
#pragma unroll
            for (int r = 0; r < 4; r++) Tb[(size_t)(64 * rb + 16 * w + 4 * r + g) * ld + col] = acc[cs][r];
        }
    }
}

// ent[2 b], ent[2 b + 1]: the range of gord that holds the non-empty groups of entry b of the view, ordered by their first member's
// row (inference_tables.h): the order of the sum does not depend on the labels.  lpd: NaN on a group whose block failed (the fill no
// kernel overwrote).  grid = (entries), one thread adds.
__global__ void __launch_bounds__(64) k_lgo_obj(MedgpDev L, const int *__restrict__ ent, const int *__restrict__ gord, const double *__restrict__ lpd) {
    const int b = blockIdx.x;
    if (L.status[b] < 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (int x = ent[2 * b]; x < ent[2 * b + 1]; x++) s += lpd[gord[x]];
    L.scal[b * 4 + 2] = -s;
}

// ------------------------------------------------------------------------------------------
// W_lgo tile + gradient block reductions: k_wgrad's prologue and phases 2 and 3, with phase 1 the product of the rows I of the full
// symmetric P and the rows J of Tt = P S over all of [0, npad) (W_lgo is symmetric: P S P = Tt P), and the LOO tile element
// G_ij - alpha_i v_j - v_i alpha_j.  QT / Q0 as in k_wgrad: 8 < Q <= 16 takes two launches, each forming G again.
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, WG_MINWAVES) k_lgo_wgrad(MedgpDev L, const double *__restrict__ vec, const double *__restrict__ Tm, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<LooElem, QT>];
    WG_PROLOGUE(false);
    const double *P = L.Kmat + (size_t)T.b * T.ld * T.ld, *Tb = Tm + (size_t)T.b * T.ld * T.ld;
    const double *vvec = vec + (size_t)T.b * 4 * T.ld + 2 * (size_t)T.ld;
    const WgAcc acc = fc_phase1(fc_zero_acc(), smem, T, P, 64 * T.I, Tb, 64 * T.J, 0, T.npad, T.I == T.J, FcNoHook(), FcNoHook());
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, LooElem{vvec});
}
