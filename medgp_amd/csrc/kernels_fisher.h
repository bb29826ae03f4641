// kernels_fisher.h -- products of the Fisher information of the Gaussian marginal likelihood with vectors (medgp_fisher_vec).
// Works behind one pipeline run that left U = L^-T (upper triangle of Linv) of every entry, and behind k_loo_kinv, which left
// P = K^-1 = U U^T as a full symmetric matrix in the entry's Kmat block.  With
//   F_hk = 1/2 tr(P dK/dtheta_h P dK/dtheta_k),     Kdot = sum_k v_k dK/dtheta_k,     T = P Kdot,     W_F = T P = P Kdot P,
//   (F v)_h = 1/2 tr(W_F dK/dtheta_h):
// the shape of the marginal-likelihood gradient with W_F in the place of W, so everything behind the W tile (block sums, wdiag,
// k_slabsum, the gradient lines of k_epilogue) is the nlml gradient's.  F does not depend on y and has no prior part.  The reference
// has no such output: the definition is tests/fisher_truth.py.
// Kdot in the numbers k_prep leaves (B_q, w_q = 2 pi mu_q, c_q = 2 (pi v_q)^2, sigma^2) and one pair (cd, sd) = cos / sin (w_q dt) by the
// angle-difference identities, e = exp(-c_q dt^2):
//   Kdot_ij = sum_q e ( (Bdot_q[m_i,m_j] + cv_q dt^2 B_q[m_i,m_j]) cd + cmu_q dt B_q[m_i,m_j] sd ) + [i == j] noise_{m_i}
//   LMC-SM  Bdot_q = Adot_q A_q^T + A_q Adot_q^T + diag(kappa_q o v_kappa),  cmu_q = -w_q v_mu,  cv_q = -2 c_q v_v,  noise_d = 2 sigma_d^2 v_sigma,d
//   SM      Bdot_q = w_q v_w (the weight),  cmu, cv, noise as above
//   SE      Bdot = 2 sf^2 v_sf,  cmu = 0,  cv = +2 c v_l (c = 1 / (2 l^2)),  noise = 2 sigma^2 v_sigma
// The noise term is never scaled by the jitter count: it is the derivative of the un-jittered K, as in the gradient calls.
//   k_fisher_prep   per entry and direction: the coefficient block  noise[D] | Bdot[Q D D] | cmu[Q] | cv[Q]  (the layout of the hyper block)
//   k_fisher_kdot   one workgroup per lower 64 x 64 tile: the Kdot tile as k_assemble_t forms K (lane = column, wave = 16-row group, one
//                   fp64 exp per pair and component); the tile and its mirror image are stored, zeros on the padding
//   k_fisher_t      one workgroup per tile of ALL tiles: T = P Kdot on fp64 MFMA (fc_phase1, two full operands, the columns of the
//                   symmetric Kdot read as rows)
//   k_fisher_wgrad  one workgroup per lower tile: G = sum_k T[i,k] P[j,k] over all of [0, npad), then k_wgrad's phases 2 and 3 with the
//                   plain tile element
// No atomics, every sum in a fixed order over operands of the entry alone: a direction's bits depend on the patient, theta and that
// direction, not on batch-mates, on the number of directions or on its position among them.
#pragma once
#include "kernels_loo_grad.h"
#include "kernels_forecast_grad.h"
#include "fisher_tables.h"

// vdir: the caller's directions [nbatch][nvec][H]; dir: the one this launch prepares.  grid = (entries, 1 + ceil(Q D D / 256)): block
// y = 0 writes noise, cmu, cv, the others one entry of Bdot per thread.  Bdot_q[i][j] is formed from (max, min) of (i, j): the same bits
// on both sides of the diagonal.
__global__ void __launch_bounds__(256) k_fisher_prep(MedgpDev L, const double *__restrict__ theta, const double *__restrict__ vdir, int nvec, int dir,
                                                     double *__restrict__ coef) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (L.status[b] < 0) return;
    const int Q = L.Q, D = L.D, R = L.R;
    const int pos = L.bpos ? L.bpos[b] : b;
    const double *th = theta + (size_t)(L.tpos ? L.tpos[b] : pos) * L.H;
    const double *v = vdir + ((size_t)pos * nvec + dir) * L.H;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *sig2 = hyp, *B = hyp + hyp_off_B(L), *w = hyp + hyp_off_w(L), *c = hyp + hyp_off_c(L);
    double *cf = coef + (size_t)b * L.hyp_stride;
    double *nd = cf, *Bd = cf + hyp_off_B(L), *cmu = cf + hyp_off_w(L), *cv = cf + hyp_off_c(L);
    if (blockIdx.y == 0) {
        if (L.kidx == 7) {
            const double *vmu = v + D + Q * D * R, *vv = vmu + Q;
            for (int d = tid; d < D; d += 256) nd[d] = 2.0 * sig2[d] * v[d];
            for (int q = tid; q < Q; q += 256) { cmu[q] = -(w[q] * vmu[q]); cv[q] = -2.0 * c[q] * vv[q]; }
        } else if (L.kidx == 8) {
            if (tid == 0) nd[0] = 2.0 * sig2[0] * v[0];
            for (int q = tid; q < Q; q += 256) { cmu[q] = -(w[q] * v[1 + Q + q]); cv[q] = -2.0 * c[q] * v[1 + 2 * Q + q]; }
        } else if (tid == 0) {
            nd[0] = 2.0 * sig2[0] * v[0];
            cmu[0] = 0.0;
            cv[0] = 2.0 * c[0] * v[1];
        }
        return;
    }
    const int idx = ((int)blockIdx.y - 1) * 256 + tid;
    if (idx >= Q * D * D) return;
    if (L.kidx == 7) {
        const double *A = th + D, *Ad = v + D, *lk = th + D + Q * (D * R + 2), *vk = v + D + Q * (D * R + 2);
        const int q = idx / (D * D), rem = idx - q * D * D, i = rem / D, j = rem - i * D;
        const int hi = max(i, j), lo = min(i, j);
        const double *Ah = A + ((size_t)q * D + hi) * R, *Al = A + ((size_t)q * D + lo) * R;
        const double *Dh = Ad + ((size_t)q * D + hi) * R, *Dl = Ad + ((size_t)q * D + lo) * R;
        double s = 0.0;
        for (int r = 0; r < R; r++) s += Dh[r] * Al[r] + Ah[r] * Dl[r];
        if (i == j) s += exp(lk[q * D + i]) * vk[q * D + i];
        Bd[idx] = s;
    } else if (L.kidx == 8) Bd[idx] = B[idx] * v[1 + idx];   // D = 1: idx = q
    else Bd[idx] = 2.0 * B[0] * v[2];
}

// ------------------------------------------------------------------------------------------
// The Kdot tile (I, J), I >= J, of one entry: k_assemble_t's loop with the direction's coefficients.  grid = (lower tiles, entries).
// QT / Q0 as in k_assemble_t: the launch <Q - 8, 8> ADDS its components to what <8, 0> stored.  The tile leaves through LDS so that it
// and its mirror image are stored as contiguous rows; a diagonal tile stores its lower half on both sides (sd = sin(w dt) from the
// tables is antisymmetric only up to rounding).  Zeros on the padding [n, npad).
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(256) k_fisher_kdot(MedgpDev L, const double *__restrict__ coef, double *__restrict__ Kdot) {
    __shared__ double Ws[64][66];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][2 + 2 * QT];
    const int b = blockIdx.y;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64), nb = npad / 64;
    int I, J;
    fisher_lower_tile(blockIdx.x, I, J);
    if (I >= nb) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = L.D;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride, *cf = coef + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L) + (size_t)Q0 * D * D, *Bd = cf + hyp_off_B(L) + (size_t)Q0 * D * D;
    const double *t = L.pt + (size_t)slot * L.pld;
    const int *meta = L.pmeta + (size_t)slot * L.pld;
    const double *csb = L.cs + ((size_t)b * L.Q + Q0) * ld, *snb = L.sn + ((size_t)b * L.Q + Q0) * ld;
    double *Kd = Kdot + (size_t)b * ld * ld;
    double cq2n[QT], cmu[QT], cv[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) {
        cq2n[q] = uniform_d(-hyp[hyp_off_c(L) + Q0 + q] * MEDGP_LOG2E);
        cmu[q] = uniform_d(cf[hyp_off_w(L) + Q0 + q]);
        cv[q] = uniform_d(cf[hyp_off_c(L) + Q0 + q]);
    }
    const int j = 64 * J + lane;
    const bool jv = j < n;
    const double tj = t[j];
    const int mj = jv ? meta[j] : 0;
    double csj[QT], snj[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) { csj[q] = csb[q * ld + j]; snj[q] = snb[q * ld + j]; }
    double bq[QT], bd[QT];
    int mcur = -1;
    const int irow = 64 * I + 16 * w + (lane & 15);
    const double r_t = t[irow];
    const int r_m = irow < n ? meta[irow] : 0;
    if (lane < 16) {
        rowc[w][lane][0] = r_t;
#pragma unroll
        for (int q = 0; q < QT; q++) { rowc[w][lane][2 + 2 * q] = csb[q * ld + irow]; rowc[w][lane][3 + 2 * q] = snb[q * ld + irow]; }
    }
    __builtin_amdgcn_wave_barrier();
    for (int rr = 0; rr < 16; rr++) {
        const int i = 64 * I + 16 * w + rr;          // wave-uniform
        double v = 0.0;
        if (i < n) {
            const int mi = __builtin_amdgcn_readlane(r_m, rr);
            if (mi != mcur) {
                mcur = mi;
#pragma unroll
                for (int q = 0; q < QT; q++) { bq[q] = B[(size_t)q * D * D + mi * D + mj]; bd[q] = Bd[(size_t)q * D * D + mi * D + mj]; }
            }
            const double dt = rowc[w][rr][0] - tj, dd = dt * dt;
            double acc = 0.0;
            if constexpr (Q0 > 0) acc = Kd[(size_t)i * ld + j];   // the components below Q0 (and the noise term) are in the tile already
#pragma unroll
            for (int q = 0; q < QT; q++) {
                const v2d csn = *(const v2d *)&rowc[w][rr][2 + 2 * q];
                const double cd = csn[0] * csj[q] + csn[1] * snj[q];
                const double sd = csn[1] * csj[q] - csn[0] * snj[q];
                const double e = exp2_nonpos(cq2n[q] * dd);
                acc += e * ((bd[q] + (cv[q] * dd) * bq[q]) * cd + ((cmu[q] * dt) * bq[q]) * sd);
            }
            if constexpr (Q0 == 0) {
                if (i == j) acc += cf[mj];
            }
            v = jv ? acc : 0.0;
        }
        Ws[16 * w + rr][lane] = v;
    }
    __syncthreads();
    for (int x = tid; x < 64 * 64; x += 256) {
        const int r = x >> 6, cc = x & 63;
        Kd[(size_t)(64 * I + r) * ld + 64 * J + cc] = (I == J && cc > r) ? Ws[cc][r] : Ws[r][cc];
        if (I != J) Kd[(size_t)(64 * J + r) * ld + 64 * I + cc] = Ws[cc][r];
    }
}

// ------------------------------------------------------------------------------------------
// T tile (I, J) of ALL tiles of the entry: sum over k in [0, npad) of P[I rows][k] Kdot[J rows][k] (Kdot is symmetric: its columns are
// read as rows, contiguous in k).  grid = (nt64^2, entries); tiles beyond the entry's own blocks exit.  P has the identity and Kdot
// zeros on the padding, so T has zeros there.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG_THREADS) k_fisher_t(MedgpDev L, const double *__restrict__ Kdot, double *__restrict__ Tm, int nt64) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    const double (*Ws)[66] = (const double (*)[66])smem;
    const int b = blockIdx.y;
    if (L.status[b] < 0) return;
    const int slot = __builtin_amdgcn_readfirstlane(L.bslot[b]);
    const int n = __builtin_amdgcn_readfirstlane(L.pn[slot]);
    const int ld = L.ldn, npad = medgp_roundup(n, 64);
    int I, J;
    fisher_t_tile(blockIdx.x, nt64, I, J);
    if (64 * I >= npad || 64 * J >= npad) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const WgTile T{b, slot, n, ld, npad, I, J, tid, lane, lane & 15, lane >> 4, __builtin_amdgcn_readfirstlane(tid >> 6)};
    const double *P = L.Kmat + (size_t)b * ld * ld, *Kd = Kdot + (size_t)b * ld * ld;
    const WgAcc acc = fc_phase1(fc_zero_acc(), smem, T, P, 64 * I, Kd, 64 * J, 0, npad, false, FcNoHook(), FcNoHook());
    wg_phase2(acc, smem, T);
    double *Tb = Tm + (size_t)b * ld * ld;
    for (int x = tid; x < 64 * 64; x += WG_THREADS) {
        const int r = x >> 6, cc = x & 63;
        Tb[(size_t)(64 * I + r) * ld + 64 * J + cc] = Ws[r][cc];
    }
}

// ------------------------------------------------------------------------------------------
// W_F tile + gradient block reductions: k_wgrad's prologue and phases 2 and 3, with phase 1 the product of the rows I of T and the rows
// J of the full symmetric P over all of [0, npad) (W_F = T P is symmetric: the lower tiles are all phase 3 reads), and the plain
// tile element.  QT / Q0 as in k_wgrad: 8 < Q <= 16 takes two launches, each forming G again.
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, WG_MINWAVES) k_fisher_wgrad(MedgpDev L, const double *__restrict__ Tm, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<FcElem, QT>];
    WG_PROLOGUE(false);
    const double *P = L.Kmat + (size_t)T.b * T.ld * T.ld, *Tb = Tm + (size_t)T.b * T.ld * T.ld;
    const WgAcc acc = fc_phase1(fc_zero_acc(), smem, T, Tb, 64 * T.I, P, 64 * T.J, 0, T.npad, T.I == T.J, FcNoHook(), FcNoHook());
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, FcElem());
}
