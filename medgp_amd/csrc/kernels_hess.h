// kernels_hess.h -- products of the exact (observed) Hessian of the data term of the nlml with vectors (medgp_hess_vec).
// Works behind one pipeline run that left U = L^-T and alpha = K^-1 y of every entry, and behind k_loo_kinv, which left P = K^-1 as a
// full symmetric matrix in the entry's Kmat block.  With  L(theta) = 1/2 y^T K^-1 y + 1/2 log det K,  W = P - alpha alpha^T,
//   Kdot = sum_k v_k dK/dtheta_k,   T = P Kdot,   beta = T alpha,   Wdot = -T P + beta alpha^T + alpha beta^T,
//   (H v)_h = 1/2 tr(Wdot dK/dtheta_h) + 1/2 tr(W dKdot/dtheta_h).
// The first term is the nlml gradient with Wdot in the place of W (k_hess_wgrad: k_fisher_wgrad with a rank-2 tile element; block
// sums, wdiag, k_slabsum as the gradient's).  The second needs second derivatives of the kernel; in block sums of W against
// k_q, km_q = dk_q/dlog mu_q, kv_q = dk_q/dlog v_q (S, SM, SV of kernels_wgrad.h) and two raw moments more,
//   M3_q[d,e] = sum W_ij e sin(w_q dt) dt^3,     M4_q[d,e] = sum W_ij e cos(w_q dt) dt^4          (e = exp(-c_q dt^2))
//   SMM = SM + (w^2 / 2c) SV,     SMV = 2 c w M3,     SVV = 2 SV + 4 c^2 M4
// which do not depend on v: the five-plane pass over W (k_hess_moments) runs once per call.  The reference has no such output: the
// definition is tests/hess_truth.py.  The lines of the epilogue (B_q, Bdot_q of k_fisher_prep; sym = the symmetric block sum):
//   sigma_d   sigma_d^2 (sum_{i in d} Wdot_ii + 2 v_sigma,d sum_{i in d} W_ii)
//   A_q       (S_q(Wdot) + v_mu SM_q(W) + v_v SV_q(W)) A_q + S_q(W) Adot_q
//   mu_q      1/2 sum Bdot_q o SM_q(W) + 1/2 sum B_q o (SM_q(Wdot) + v_mu SMM_q + v_v SMV_q)
//   v_q       1/2 sum Bdot_q o SV_q(W) + 1/2 sum B_q o (SV_q(Wdot) + v_mu SMV_q + v_v SVV_q)
//   kappa_qd  1/2 kappa_qd (v_kappa S_q(W)[d,d] + S_q(Wdot)[d,d] + v_mu SM_q(W)[d,d] + v_v SV_q(W)[d,d])
//   SM        the mu / v lines with 1 x 1 blocks, B = the weight, Bdot = B v_w; the weight: 1/2 B (S(Wdot) + v_w S + v_mu SM + v_v SV)
//   SE        l: 1/2 B (-SV(Wdot) + v_l SVV - 2 v_sf SV);   sf: B (S(Wdot) - v_l SV + 2 v_sf S)        (d/dlog l = -d/dlog v)
// The noise terms are never scaled by the jitter count.
//   k_hess_moments  one workgroup per lower tile: k_wgrad's phases 1 and 2 (U U^T) and its phase 3 with the nlml element (S, SM, SV
//                   pieces -> slab, diag(W) -> wdiag of the view it is given), then a second pass over the tile in LDS for the pieces
//                   of M3 and M4 -> a slab of the call with two planes and the same R x C geometry.  Pieces written once, no atomics.
//   k_hess_slabsum  k_slabsum for those two planes
//   k_hess_beta     beta = T alpha, 16-row blocks, lanes stride over the columns, fixed butterfly
//   k_hess_wgrad    one workgroup per lower tile: G = T P over all of [0, npad), the element -G_ij + beta_i alpha_j + alpha_i beta_j,
//                   k_wgrad's phases 2 and 3
//   k_hess_epilogue per (entry, direction): the lines above, hyper range chunked over parts as k_epilogue
// No atomics, every sum in a fixed order over operands of the entry alone: a direction's bits depend on the patient, theta and that
// direction, not on batch-mates, on the number of directions or on its position among them.
#pragma once
#include "kernels_fisher.h"
#include "hess_tables.h"

// Workgroups per SIMD the tile kernels promise the compiler.  At k_wgrad's three the widest instantiations do not fit 168 VGPRs
// and would spill to scratch (as k_wgrad<8> itself does); two leave them 256.
constexpr int hess_moments_minwaves(int QT) { return QT >= 6 ? 2 : WG_MINWAVES; }
constexpr int hess_wgrad_minwaves(int QT) { return QT >= 8 ? 2 : WG_MINWAVES; }

// phase-3 element of k_hess_wgrad: -G_ij + beta_i alpha_j + alpha_i beta_j; the row and column constants carry beta beside alpha
struct HessElem {
    static constexpr int NX = 1;
    const double *beta;
    __device__ __forceinline__ double extra(int k) const { return beta[k]; }
    __device__ __forceinline__ double elem(double ws, double ai, double aj, double bi, double bj) const { return (bi * aj - ws) + ai * bj; }
};

// The second pass of k_hess_moments over the W tile left in Ws by wg_phase2: wg_phase3's loop, flush and slab addressing with the nlml
// element and the two running sums  sum w e sd dt^3,  sum w e cd dt^4  per component; hi: the entry's two planes [2][Q][R][C].
template <int QT, int Q0>
__device__ __forceinline__ void hess_phase3_hi(const MedgpDev &L, const WgTile T, const double *smem, double (*rowc)[16][2 + 2 * QT], double *__restrict__ hi) {
    const double (*Ws)[66] = (const double (*)[66])smem;
    const int b = T.b, slot = T.slot, n = T.n, ld = T.ld, I = T.I, J = T.J, lane = T.lane, w = T.w;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *t = L.pt + (size_t)slot * L.pld;
    const int *meta = L.pmeta + (size_t)slot * L.pld;
    const double *alpha = L.alpha + (size_t)b * ld;
    const int *seg = L.pseg + (size_t)slot * (L.D + 1);
    const int *roff = L.proff + (size_t)slot * (L.D + 1), *coff = L.pcoff + (size_t)slot * (L.D + 1);
    const double *csb = L.cs + ((size_t)b * L.Q + Q0) * ld, *snb = L.sn + ((size_t)b * L.Q + Q0) * ld;
    const int Qall = L.Q, Rmax = L.slab_R, Cmax = L.slab_C;
    double cq2n[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) cq2n[q] = uniform_d(-hyp[hyp_off_c(L) + Q0 + q] * MEDGP_LOG2E);
    const int j = 64 * J + lane;
    const bool jv = j < n;
    const double tj = t[j], aj = alpha[j];
    const int mj = jv ? meta[j] : -1;
    double csj[QT], snj[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) { csj[q] = csb[q * ld + j]; snj[q] = snb[q * ld + j]; }
    const int mprev = __shfl_up(mj, 1);
    const bool leader = (lane == 0) || (mj != mprev);
    const unsigned long long lmask = __ballot(leader);
    int segend;
    {
        unsigned long long above = (lane == 63) ? 0ull : (lmask >> (lane + 1));
        segend = above ? (lane + 1 + __builtin_ctzll(above)) : 64;
    }
    const unsigned long long upto = lmask & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
    const int segstart = 63 - __builtin_clzll(upto);
    const bool seglast = (lane == segend - 1);
    const int cslot = (mj >= 0) ? coff[mj] + (J - seg[mj] / 64) : 0;
    const int rg = 4 * I + w;

    double s3[QT], s4[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) { s3[q] = 0.0; s4[q] = 0.0; }
    int mcur = -2;
    const int irow = 64 * I + 16 * w + (lane & 15);
    const int r_m = (irow < n) ? meta[irow] : -1;
    __builtin_amdgcn_wave_barrier();   // (the wave's reads of rowc in the first pass are done)
    if (lane < 16) {
        rowc[w][lane][0] = t[irow]; rowc[w][lane][1] = alpha[irow];
#pragma unroll
        for (int q = 0; q < QT; q++) { rowc[w][lane][2 + 2 * q] = csb[q * ld + irow]; rowc[w][lane][3 + 2 * q] = snb[q * ld + irow]; }
    }
    __builtin_amdgcn_wave_barrier();
    for (int rr = 0; rr <= 16; rr++) {
        const int i = 64 * I + 16 * w + rr;
        int mi = -1;
        if (rr < 16) mi = __builtin_amdgcn_readlane(r_m, rr);          // wave-uniform
        if (mi != mcur) {
            if (mcur >= 0) {
                const int rslot = roff[mcur] + (rg - seg[mcur] / 16);
                double fv[2 * QT];
#pragma unroll
                for (int q = 0; q < QT; q++) { fv[q] = s3[q]; fv[QT + q] = s4[q]; }
#pragma unroll
                for (int dlt = 1; dlt < 64; dlt <<= 1) {
                    double up[2 * QT];
#pragma unroll
                    for (int k = 0; k < 2 * QT; k++) up[k] = __shfl_up(fv[k], dlt);
                    if (lane - dlt >= segstart) {
#pragma unroll
                        for (int k = 0; k < 2 * QT; k++) fv[k] += up[k];
                    }
                }
                if (seglast && mj >= 0) {
#pragma unroll
                    for (int k = 0; k < 2 * QT; k++) hi[((size_t)((k / QT) * Qall + Q0 + (k % QT)) * Rmax + rslot) * Cmax + cslot] = fv[k];
                }
            }
#pragma unroll
            for (int q = 0; q < QT; q++) { s3[q] = 0.0; s4[q] = 0.0; }
            mcur = mi;
        }
        if (rr == 16 || mi < 0) continue;
        const v2d ta = *(const v2d *)&rowc[w][rr][0];
        const double ti = ta[0], ai = ta[1];
        double wv = Ws[16 * w + rr][lane] - ai * aj;
        const bool valid = jv && (j <= i);
        wv = valid ? ((mi == mj && j < i) ? 2.0 * wv : wv) : 0.0;
        const double dt = ti - tj, dd = dt * dt;
#pragma unroll
        for (int q = 0; q < QT; q++) {
            const v2d csn = *(const v2d *)&rowc[w][rr][2 + 2 * q];
            const double ci = csn[0], si = csn[1];
            const double we = (wv * exp2_nonpos(cq2n[q] * dd)) * dd;
            const double cd = ci * csj[q] + si * snj[q];
            const double sd = si * csj[q] - ci * snj[q];
            s3[q] += (we * sd) * dt;
            s4[q] += (we * cd) * dd;
        }
    }
}

// ------------------------------------------------------------------------------------------
// The five-plane pass over W.  L is the view of the W pass: its slab takes the S, SM, SV pieces and its wdiag diag(W).  QT / Q0 as in
// k_wgrad: 8 < Q <= 16 takes two launches, each forming the tile again.
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, hess_moments_minwaves(QT)) k_hess_moments(MedgpDev L, double *__restrict__ hislab, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<WgElemNlml, QT>];
    WG_PROLOGUE(false);
    const double *U = L.Linv + (size_t)T.b * T.ld * T.ld;
    const WgAcc acc = wg_phase1<true>(smem, T, U, 64 * T.I, WgNoHook());
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, WgElemNlml());
    hess_phase3_hi<QT, Q0>(L, T, smem, rowc, hislab + (size_t)T.b * hess_hislab_stride(L.Q, L.slab_R, L.slab_C));
}

// block sums M3, M4 from the pieces of the two-plane slab, in k_slabsum's order.  grid = (nbatch, ceil(2 Q D(D+1)/2 / 256));
// sums: the class's [M3 | M4] blocks, each [entries][Q D D]
__global__ void __launch_bounds__(256) k_hess_slabsum(MedgpDev L, const double *__restrict__ hislab, double *__restrict__ M3, double *__restrict__ M4) {
    __shared__ int s_roff[MEDGP_MAX_D + 1], s_coff[MEDGP_MAX_D + 1], s_seg[MEDGP_MAX_D + 1];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    if (L.status[b] < 0) return;
    const int Q = L.Q, D = L.D;
    const int slot = L.bslot[b];
    for (int i = tid; i <= D; i += nt) {
        s_roff[i] = L.proff[(size_t)slot * (D + 1) + i];
        s_coff[i] = L.pcoff[(size_t)slot * (D + 1) + i];
        s_seg[i] = L.pseg[(size_t)slot * (D + 1) + i];
    }
    __syncthreads();
    const int nbins = D * (D + 1) / 2;
    const int idx = blockIdx.y * nt + tid;
    if (idx >= 2 * Q * nbins) return;
    const int pq = idx / nbins;          // plane * Q + q
    int d, e;
    tile_decode(idx - pq * nbins, d, e);
    const double *sl = hislab + (size_t)b * hess_hislab_stride(Q, L.slab_R, L.slab_C) + (size_t)pq * L.slab_R * L.slab_C;
    double s = 0.0;
    for (int rs = s_roff[d]; rs < s_roff[d + 1]; rs++) {
        const int It = (s_seg[d] / 16 + (rs - s_roff[d])) / 4;
        for (int cs = s_coff[e]; cs < s_coff[e + 1]; cs++) {
            const int Jt = s_seg[e] / 64 + (cs - s_coff[e]);
            if (Jt <= It) s += sl[(size_t)rs * L.slab_C + cs];
        }
    }
    const int pl = pq / Q, q = pq - pl * Q;
    (pl == 0 ? M3 : M4)[(size_t)b * Q * D * D + (size_t)q * D * D + d * D + e] = s;
}

// beta_i = sum_{k < n} T[i][k] alpha_k, zeros on the padding.  grid = (16-row blocks, entries), wave w of a workgroup owns 4 rows.
__global__ void __launch_bounds__(256) k_hess_beta(MedgpDev L, const double *__restrict__ Tm, double *__restrict__ beta) {
    const int b = blockIdx.y, rb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    if (16 * rb >= npad) return;
    const int r0 = 16 * rb + 4 * w;
    const double *Tr = Tm + (size_t)b * ld * ld + (size_t)r0 * ld, *al = L.alpha + (size_t)b * ld;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k < n; k += 64) {
        const double a = al[k];
#pragma unroll
        for (int e = 0; e < 4; e++) s[e] += Tr[(size_t)e * ld + k] * a;
    }
#pragma unroll
    for (int e = 0; e < 4; e++)
        for (int off = 32; off > 0; off >>= 1) s[e] += __shfl_xor(s[e], off);
    if (lane < 4) {
        const int i = r0 + lane;
        const double v = lane == 0 ? s[0] : (lane == 1 ? s[1] : (lane == 2 ? s[2] : s[3]));
        beta[(size_t)b * ld + i] = (i < n) ? v : 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// Wdot tile + gradient block reductions: k_fisher_wgrad with the rank-2 element (alpha from L.alpha, beta of the class view).
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, hess_wgrad_minwaves(QT)) k_hess_wgrad(MedgpDev L, const double *__restrict__ Tm, const double *__restrict__ beta, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<HessElem, QT>];
    WG_PROLOGUE(false);
    const double *P = L.Kmat + (size_t)T.b * T.ld * T.ld, *Tb = Tm + (size_t)T.b * T.ld * T.ld;
    const WgAcc acc = fc_phase1(fc_zero_acc(), smem, T, Tb, 64 * T.I, P, 64 * T.J, 0, T.npad, T.I == T.J, FcNoHook(), FcNoHook());
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, HessElem{beta + (size_t)T.b * T.ld});
}

// what the W pass left, per class view: block sums [entries][Q D D] and diag(W) [entries][ld]
struct HessW { const double *S, *SM, *SV, *M3, *M4, *wdiag; };

// ------------------------------------------------------------------------------------------
// The lines of the header for direction `dir` of every entry.  L: the direction's view (S, SM, SV, wdiag of Wdot); hw: the W pass.
// grid = (entries, parts), the hyper range cut as in k_epilogue.  out: this direction's rows [nbatch][H] (caller rows).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_hess_epilogue(MedgpDev L, HessW hw, const double *__restrict__ theta, const double *__restrict__ vdir, int nvec,
                                                       int dir, const double *__restrict__ coef, double *__restrict__ out, int *__restrict__ status_out) {
    __shared__ double smuv[2 * 16], s_sig[2][MEDGP_MAX_D];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, nwave = nt >> 6;
    const int H = L.H, Q = L.Q, D = L.D, R = L.R, ld = L.ldn;
    const int part = blockIdx.y, nparts = gridDim.y;
    const int nchunk = min(MEDGP_EPI_PARTS, (H + 255) / 256), hchunk = (H + nchunk - 1) / nchunk;
    const int cpp = (nchunk + nparts - 1) / nparts, ch0 = part * cpp, ch1 = min(nchunk, ch0 + cpp);
    const int h0 = ch0 * hchunk, h1 = min(H, ch1 * hchunk);
    const int st = L.status[b];
    const int pos = L.bpos ? L.bpos[b] : b;
    double *g = out + (size_t)pos * H;
    if (tid == 0 && part == 0 && status_out) status_out[pos] = st;
    if (st < 0) {
        for (int h = h0 + tid; h < h1; h += nt) g[h] = __builtin_nan("");
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot];
    const double *th = theta + (size_t)(L.tpos ? L.tpos[b] : pos) * H;
    const double *v = vdir + ((size_t)pos * nvec + dir) * H;
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride, *cf = coef + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *Bd = cf + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L);
    const size_t qdd = (size_t)b * Q * D * D;
    const double *Sd = L.S + qdd, *SMd = L.SM + qdd, *SVd = L.SV + qdd;                                          // of Wdot
    const double *S = hw.S + qdd, *SM = hw.SM + qdd, *SV = hw.SV + qdd, *M3 = hw.M3 + qdd, *M4 = hw.M4 + qdd;    // of W
    const double *Wdd = L.wdiag + (size_t)b * ld, *Wd = hw.wdiag + (size_t)b * ld;
    const int *seg = L.pseg + (size_t)slot * (D + 1);
    // where mu | v | (SM: the weights) start in theta, and the direction's components there
    const int o_mu = L.kidx == 7 ? D + Q * D * R : 1 + Q, o_v = o_mu + Q;
    if (L.kidx != 0) {
        // the 2Q frequency / length-scale lines are D(D+1)/2-term contractions: one wave each, lanes stride over the bins, fixed butterfly
        const int nbins = D * (D + 1) / 2;
        for (int w2 = tid >> 6; w2 < 2 * Q; w2 += nwave) {
            const bool is_mu = w2 < Q;
            const int q = is_mu ? w2 : w2 - Q;
            if (o_mu + w2 < h0 || o_mu + w2 >= h1) continue;   // wave-uniform: not this part's hyper
            const double vmu = v[o_mu + q], vv = v[o_v + q], w = wq[q], c = cq[q];
            const double *Bq = B + (size_t)q * D * D, *Bdq = Bd + (size_t)q * D * D;
            const size_t o = (size_t)q * D * D;
            double sacc = 0.0;
            int d, e;
            tile_decode(lane, d, e);
            for (int idx = lane; idx < nbins; idx += 64) {
                const int x = d * D + e;
                const double smv = (2.0 * c * w) * M3[o + x];
                double line;
                if (is_mu) line = Bdq[x] * SM[o + x] + Bq[x] * (SMd[o + x] + vmu * (SM[o + x] + (w * w / (2.0 * c)) * SV[o + x]) + vv * smv);
                else line = Bdq[x] * SV[o + x] + Bq[x] * (SVd[o + x] + vmu * smv + vv * (2.0 * SV[o + x] + (4.0 * c * c) * M4[o + x]));
                sacc += ((d == e) ? 1.0 : 2.0) * line;
                e += 64;
                while (e > d) { e -= d + 1; d++; }
            }
            for (int off = 32; off > 0; off >>= 1) sacc += __shfl_xor(sacc, off);
            if (lane == 0) smuv[w2] = sacc;
        }
    }
    {
        // the noise lines: sums of diag(Wdot) and diag(W) over the observations of one output, one wave each
        const int nl = L.kidx == 7 ? D : 1, dhi = min(nl, h1);
        for (int d = h0 + (tid >> 6); d < dhi; d += nwave) {
            const int i0 = L.kidx == 7 ? seg[d] : 0, i1 = L.kidx == 7 ? seg[d + 1] : n;
            double sa = 0.0, sb = 0.0;
            for (int i = i0 + lane; i < i1; i += 64) { sa += Wdd[i]; sb += Wd[i]; }
            for (int off = 32; off > 0; off >>= 1) { sa += __shfl_xor(sa, off); sb += __shfl_xor(sb, off); }
            if (lane == 0) { s_sig[0][d] = sa; s_sig[1][d] = sb; }
        }
    }
    __syncthreads();
    for (int h = h0 + tid; h < h1; h += nt) {
        double gv;
        const int nl = L.kidx == 7 ? D : 1;
        if (h < nl) {
            const double hv = exp(th[h]);
            gv = (hv * hv) * (s_sig[0][h] + (2.0 * v[h]) * s_sig[1][h]);
        } else if (L.kidx == 7) {
            const int hc = h - D;
            if (hc < Q * D * R) {
                const int q = hc / (D * R), rem = hc - q * D * R, d = rem / R, r = rem - d * R;
                const double *A = th + D + (size_t)q * D * R, *Ad = v + D + (size_t)q * D * R;
                const size_t o = (size_t)q * D * D;
                const double vmu = v[o_mu + q], vv = v[o_v + q];
                double s = 0.0;
                for (int e = 0; e < D; e++) {
                    const int x = (d >= e) ? d * D + e : e * D + d;
                    s += (Sd[o + x] + (vmu * SM[o + x] + vv * SV[o + x])) * A[e * R + r] + S[o + x] * Ad[e * R + r];
                }
                gv = s;
            } else if (hc < Q * (D * R + 2)) gv = 0.5 * smuv[hc - Q * D * R];
            else {
                const int kk = hc - Q * (D * R + 2), q = kk / D, d = kk - q * D;
                const size_t x = (size_t)q * D * D + d * D + d;
                gv = 0.5 * exp(th[h]) * (v[h] * S[x] + (Sd[x] + (v[o_mu + q] * SM[x] + v[o_v + q] * SV[x])));
            }
        } else if (L.kidx == 8) {
            const int hc = h - 1, mode = hc / Q, q = hc - mode * Q;
            if (mode == 0) gv = 0.5 * B[q] * (Sd[q] + (v[1 + q] * S[q] + v[o_mu + q] * SM[q] + v[o_v + q] * SV[q]));
            else gv = 0.5 * smuv[hc - Q];
        } else {
            const double c = cq[0], svv = 2.0 * SV[0] + (4.0 * c * c) * M4[0];
            if (h == 1) gv = 0.5 * B[0] * (v[1] * svv - 2.0 * v[2] * SV[0] - SVd[0]);
            else gv = B[0] * (Sd[0] + (2.0 * v[2] * S[0] - v[1] * SV[0]));
        }
        g[h] = gv;
    }
}
