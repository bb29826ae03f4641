// kernels_forecast_grad.h -- the negative h-hours-ahead forecast score and its hyper-parameter gradient (medgp_forecast_grad).
// Works behind one pipeline run in the CALLER's order that left L (lower triangle of Kmat), z = L^-1 y and U = L^-T (upper triangle
// of Linv) of every entry.  Scored observation i is predicted from the leading block obs[0 : p_i], p_i <= i:
//   var_i = sum_{k = p_i .. i} L[i,k]^2,   r_i = sum_{k = p_i .. i} L[i,k] z[k],   lpd_i = -1/2 log(2 pi var_i) - 1/2 r_i^2 / var_i,
//   J = - sum_i lpd_i,      g_i = (1 - r_i^2 / var_i) / var_i,      e_i = r_i / var_i,
//   dJ / d theta_h = 1/2 tr(W_fc dK / d theta_h),     W_fc = T Qm^T + Qm T^T,
//   T = U Mbar      Mbar[k,i] = L[i,k] on the band p_i <= k <= i, 0 elsewhere   (column i of T is u_i = [-a_i | 0 .. 0 | 1 at i | 0 ..])
//   Qm = T diag(g / 2) - B,     B[j,i] = e_i sum_{j <= k < p_i} U[j,k] z[k]      (column i of B is e_i K[0:p,0:p]^-1 y[0:p], padded)
// -- the shape of the marginal-likelihood gradient with W_fc in the place of W, so everything behind the W tile (block sums, wdiag,
// k_slabsum, k_epilogue) is the nlml gradient's.  The reference has no such output: the definition is tests/forecast_grad_truth.py.
//   k_fc_vec     mode 0: var, r, g / 2, e and lpd of a 16-row block (zeros on unscored and padding rows); mode 1: J -> scal[2]
//   k_fc_t       one workgroup per 64 x 64 tile (rows j, columns i) of T on fp64 MFMA; the columns k of the product start at the
//                band's first column of the tile (pmin); tiles below the diagonal and tiles without a scored column are zeros.
//                The ROWS are stored at their positions of the grouped order (gpos): the sum in W_fc runs over the scored index, so
//                the gradient's tile phases work against the grouped patient rows without knowing that the factor was not.
//   k_fc_scan    row j of U diag(z) -> its running sums over [j, pall), IN PLACE (U is dead behind k_fc_t)
//   k_fc_qm      Qm, element by element, into the entry's Kmat block (L is dead behind k_fc_t and k_fc_vec), rows at gpos
//   k_fc_tables  the cos / sin tables of the entries again, for the grouped copy of the patient (the host points bslot there first)
//   k_fc_wgrad   one workgroup per lower tile (I, J) of the grouped order: T_I Qm_J^T + Qm_I T_J^T over the scored column blocks, two
//                passes into one accumulator, then k_wgrad's phases 2 and 3 with the plain tile element
// No atomics, every sum in a fixed order over operands of the entry alone: an entry's bits do not depend on its batch-mates.
// Per-entry vectors (a buffer of the call): [g / 2 | e | lpd | -], 4 ld doubles per entry; the integer table: forecast_grad_tables.h.
// fc_phase1 is wg_phase1 (kernels_wgrad.h) for two different operand matrices and a column range [k0, k1); wg_phase1 itself, which
// k_wgrad and the LOO kernels share, is left as it is.
#pragma once
#include "kernels_wgrad.h"
#include "forecast_grad_tables.h"

// the table of entry b of a class view (tab: the class's first entry)
struct FcTab {
    const int *pfx, *gpos, *pmin, *pmax;
    int c0, c1, pall;
};
__device__ __forceinline__ FcTab fc_tab(const int *__restrict__ tab, int b, int ld) {
    const int *e = tab + (size_t)b * FC_TAB_INTS * ld, *blk = e + 2 * (size_t)ld;
    const int nblk = ld / 64;
    return FcTab{e, e + ld, blk, blk + nblk, blk[2 * nblk], blk[2 * nblk + 1], blk[2 * nblk + 2]};
}

// fragment hooks of fc_phase1: two adjacent doubles at column `col` of row `row`
struct FcNoHook {
    __device__ __forceinline__ v2d operator()(v2d x, int, int) const { return x; }
};
// rows of U: what lies left of the diagonal is a leftover of the factorisation
struct FcUpperHook {
    __device__ __forceinline__ v2d operator()(v2d x, int row, int col) const {
        x[0] = (col >= row) ? x[0] : 0.0;
        x[1] = (col + 1 >= row) ? x[1] : 0.0;
        return x;
    }
};
// rows of L on their band [p_i, i] (an unscored row: nothing)
struct FcBandHook {
    const int *pfx;
    __device__ __forceinline__ v2d operator()(v2d x, int row, int col) const {
        const int p = pfx[row], lo = p < 0 ? INT_MAX : p;
        x[0] = (col >= lo && col <= row) ? x[0] : 0.0;
        x[1] = (col + 1 >= lo && col + 1 <= row) ? x[1] : 0.0;
        return x;
    }
};

// acc += A[rowa0 .. +64][k] B[rowb0 .. +64][k] over the columns k0 <= k < k1 (multiples of WG_KC): the rows of B are staged through
// LDS and shared by the four waves, the rows of A stream from HBM, one chunk prefetched ahead -- wg_phase1's loop.  tri: the tile is a
// diagonal one of a symmetric result, the column strips right of a wave's rows are left out.  Ends behind a barrier.
template <class HookA, class HookB>
__device__ __forceinline__ WgAcc fc_phase1(const WgAcc in, double *smem, const WgTile T, const double *A, int rowa0, const double *B, int rowb0,
                                           int k0, int k1, bool tri, const HookA ha, const HookB hb) {
    double (*Bs)[64][WG_KC + 2] = (double (*)[64][WG_KC + 2])smem;   // Bs[2][64][34]
    v4d acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[ct] = in.a[ct];
    const int nch = (k1 - k0) / WG_KC;   // workgroup-uniform
    if (nch > 0) {
        const int ctmax = tri ? T.w : 3;   // wave-uniform
        const int li = T.li, g = T.g;
        const int srow = T.tid >> 2, scg = (T.tid & 3) * 8;
        const int arow = rowa0 + 16 * T.w + li, brow = rowb0 + srow;
        const double *Arow = A + (size_t)arow * T.ld + k0 + 2 * g;
        const double *Bsrc = B + (size_t)brow * T.ld + k0 + scg;
        v2d bst[4], an[4];
#pragma unroll
        for (int u = 0; u < 4; u++) bst[u] = hb(*(const v2d *)(Bsrc + 2 * u), brow, k0 + scg + 2 * u);
#pragma unroll
        for (int h = 0; h < 4; h++) an[h] = ha(*(const v2d *)(Arow + 8 * h), arow, k0 + 2 * g + 8 * h);
#pragma unroll
        for (int u = 0; u < 4; u++) *(v2d *)&Bs[0][srow][scg + 2 * u] = bst[u];
        __syncthreads();
        for (int c = 0; c < nch; c++) {
            const int buf = c & 1;
            v2d ac[4];
#pragma unroll
            for (int h = 0; h < 4; h++) ac[h] = an[h];
            if (c + 1 < nch) {
                const int kc = (c + 1) * WG_KC;
#pragma unroll
                for (int u = 0; u < 4; u++) bst[u] = hb(*(const v2d *)(Bsrc + kc + 2 * u), brow, k0 + kc + scg + 2 * u);
#pragma unroll
                for (int h = 0; h < 4; h++) an[h] = ha(*(const v2d *)(Arow + kc + 8 * h), arow, k0 + kc + 2 * g + 8 * h);
            }
            WG_CHUNK_MFMA(ac, buf);
            if (c + 1 < nch) {
#pragma unroll
                for (int u = 0; u < 4; u++) *(v2d *)&Bs[buf ^ 1][srow][scg + 2 * u] = bst[u];
            }
            __syncthreads();
        }
    }
    return WgAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

__device__ __forceinline__ WgAcc fc_zero_acc() {
    const v4d z = (v4d){0.0, 0.0, 0.0, 0.0};
    return WgAcc{{z, z, z, z}};
}

// ------------------------------------------------------------------------------------------
// The vectors of an entry; vec = [g / 2 | e | lpd | -] of the class view, 4 ld doubles per entry.
//   mode 0: grid = (16-row blocks, entries); wave w of a workgroup owns 4 rows, one after the other: the lanes stride over the band
//           [p_i, i] of the row from the band's first 64-block on and add their 64 partial sums by a butterfly
//   mode 1: grid = (1, entries): J = - sum_i lpd_i; thread t adds the observations t, t + 256, ..., the 256 sums go through one tree
// Both objective-only and gradient calls run exactly these two launches: the same bits of J.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fc_vec(MedgpDev L, double *__restrict__ vec, const int *__restrict__ tab, int mode, double log2pi) {
    __shared__ double red[256];
    const int b = blockIdx.y, rb = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    double *gh = vec + (size_t)b * 4 * ld, *ev = gh + ld, *lp = ev + ld;
    if (mode == 0) {
        if (16 * rb >= npad) return;
        const FcTab F = fc_tab(tab, b, ld);
        const double *Lm = L.Kmat + (size_t)b * ld * ld, *z = L.z + (size_t)b * ld;
        for (int e = 0; e < 4; e++) {
            const int i = 16 * rb + 4 * w + e;   // wave-uniform
            const int p = F.pfx[i];
            if (p < 0) {   // not scored, or padding
                if (lane == 0) { gh[i] = 0.0; ev[i] = 0.0; lp[i] = 0.0; }
                continue;
            }
            const double *row = Lm + (size_t)i * ld;
            double sv = 0.0, sr = 0.0;
            for (int k = (p & ~63) + lane; k <= i; k += 64) {
                const double l = (k >= p) ? row[k] : 0.0;
                sv += l * l;
                sr += l * z[k];
            }
            for (int off = 32; off > 0; off >>= 1) { sv += __shfl_xor(sv, off); sr += __shfl_xor(sr, off); }
            if (lane == 0) {
                const double q = sr * sr / sv;
                gh[i] = 0.5 * ((1.0 - q) / sv);
                ev[i] = sr / sv;
                lp[i] = -0.5 * (log(sv) + log2pi) - 0.5 * q;
            }
        }
        return;
    }
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
// T tile (R, C): rows j of block R, columns i of block C: sum over k of U[j,k] Mbar[i,k], k from the later of the block's first row
// and the band's first column (rounded down to a chunk) to the end of block C.  grid = (nt64^2, entries).  The tile leaves through LDS,
// row r to row gpos[64 R + r] of Tm (the class's matrices, laid out like Kmat).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WG_THREADS) k_fc_t(MedgpDev L, double *__restrict__ Tm, const int *__restrict__ tab, int nt64) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    double (*Ws)[66] = (double (*)[66])smem;   // Ws[64][66]
    const int b = blockIdx.y;
    if (L.status[b] < 0) return;
    const int slot = __builtin_amdgcn_readfirstlane(L.bslot[b]);
    const int n = __builtin_amdgcn_readfirstlane(L.pn[slot]);
    const int ld = L.ldn, npad = medgp_roundup(n, 64);
    const int R = blockIdx.x / nt64, C = blockIdx.x - R * nt64;
    if (64 * R >= npad || 64 * C >= npad) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const WgTile T{b, slot, n, ld, npad, R, C, tid, lane, lane & 15, lane >> 4, __builtin_amdgcn_readfirstlane(tid >> 6)};
    const FcTab F = fc_tab(tab, b, ld);
    const int pmin = F.pmin[C];
    const bool active = R <= C && pmin != FC_EMPTY_MIN;   // workgroup-uniform
    if (active) {
        const int k0 = max(64 * R, pmin & ~(WG_KC - 1)), k1 = 64 * C + 64;
        const double *U = L.Linv + (size_t)b * ld * ld, *Lm = L.Kmat + (size_t)b * ld * ld;
        const WgAcc acc = fc_phase1(fc_zero_acc(), smem, T, U, 64 * R, Lm, 64 * C, k0, k1, false, FcUpperHook(), FcBandHook{F.pfx});
        wg_phase2(acc, smem, T);
    }
    double *Tb = Tm + (size_t)b * ld * ld;
    for (int x = tid; x < 64 * 64; x += WG_THREADS) {
        const int r = x >> 6, cc = x & 63;
        Tb[(size_t)F.gpos[64 * R + r] * ld + 64 * C + cc] = active ? Ws[r][cc] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------
// Row j of U diag(z) -> S[j,k] = sum_{j <= k' <= k} U[j,k'] z[k'] for k in [j, pall), in place.  One wave per row, 64 columns at a
// time: an inclusive scan over the lanes (6 shuffle steps, fixed order) plus the carry of the chunks before.  Rows j >= pall are never
// read (beta_i lives on [0, p_i)).  grid = (ceil(npad / 4), entries).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fc_scan(MedgpDev L, const int *__restrict__ tab) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, j = 4 * blockIdx.x + (threadIdx.x >> 6);
    if (L.status[b] < 0) return;
    const int ld = L.ldn;
    const FcTab F = fc_tab(tab, b, ld);
    if (j >= F.pall) return;   // (pall <= n - 1)
    double *row = L.Linv + (size_t)b * ld * ld + (size_t)j * ld;
    const double *z = L.z + (size_t)b * ld;
    double carry = 0.0;
    for (int k0 = j & ~63; k0 < F.pall; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k >= j && k < F.pall;
        double v = in ? row[k] * z[k] : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double up = __shfl_up(v, d);
            if (lane >= d) v += up;
        }
        v += carry;
        if (in) row[k] = v;
        carry = __shfl(v, 63);
    }
}

// ------------------------------------------------------------------------------------------
// Qm[j,i] = T[j,i] g_i / 2 - e_i S[j, p_i - 1] (the last term for j < p_i only), zero for unscored columns and below the diagonal;
// rows at gpos.  grid = (column blocks, 4-row groups, entries); S = the scanned rows of Linv, the result goes to the Kmat block.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fc_qm(MedgpDev L, const double *__restrict__ Tm, const double *__restrict__ vec, const int *__restrict__ tab) {
    const int b = blockIdx.z;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const int i = 64 * blockIdx.x + (threadIdx.x & 63), j = 4 * blockIdx.y + (threadIdx.x >> 6);
    if (i >= npad || j >= npad) return;
    const FcTab F = fc_tab(tab, b, ld);
    const double *gh = vec + (size_t)b * 4 * ld, *ev = gh + ld;
    const double *S = L.Linv + (size_t)b * ld * ld, *Tb = Tm + (size_t)b * ld * ld;
    double *Qm = L.Kmat + (size_t)b * ld * ld;
    const int p = F.pfx[i];
    const size_t at = (size_t)F.gpos[j] * ld + i;
    double val = 0.0;
    if (p >= 0 && j <= i) {
        const double beta = (j < p) ? S[(size_t)j * ld + p - 1] : 0.0;
        val = Tb[at] * gh[i] - ev[i] * beta;
    }
    Qm[at] = val;
}

// ------------------------------------------------------------------------------------------
// The cos / sin tables of every entry of the view for the patient copy bslot names NOW (the grouped one): k_prep's table blocks with
// w_q read from the entry's hyper block (where k_prep stored the very value it used), and nothing else of k_prep -- status, jitter
// count and the scalars of the factorisation stay.  grid = (entries, table chunks of PREP_CHUNK).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fc_tables(MedgpDev L) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int slot = L.bslot[b], n = L.pn[slot], Q = L.Q;
    const double *w = L.hyp + (size_t)b * L.hyp_stride + hyp_off_w(L);
    const double *t = L.pt + (size_t)slot * L.pld;
    double *cs = L.cs + (size_t)b * Q * L.ldn, *sn = L.sn + (size_t)b * Q * L.ldn;
    const int lo = blockIdx.y * PREP_CHUNK, hi = min(lo + PREP_CHUNK, Q * L.ldn);
    for (int idx = lo + tid; idx < hi; idx += 256) {
        const int q = idx / L.ldn, i = idx - q * L.ldn;
        double s = 0.0, co = 0.0;
        if (i < n) sincos(w[q] * t[i], &s, &co);
        cs[idx] = co;
        sn[idx] = s;
    }
}

// phase-3 element of k_fc_wgrad: the accumulated tile is W_fc itself
struct FcElem {
    static constexpr int NX = 0;
    __device__ __forceinline__ double extra(int) const { return 0.0; }
    __device__ __forceinline__ double elem(double ws, double, double, double, double) const { return ws; }
};

// ------------------------------------------------------------------------------------------
// W_fc tile + gradient block reductions: k_wgrad's prologue and phases 2 and 3, with phase 1 the two products T_I Qm_J^T and
// Qm_I T_J^T over the column blocks [c0, c1) that hold scored observations (T and Qm are zero elsewhere).  Rows are grouped rows.
// QT / Q0 as in k_wgrad: 8 < Q <= 16 takes two launches, each forming the tile again.
// ------------------------------------------------------------------------------------------
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, WG_MINWAVES) k_fc_wgrad(MedgpDev L, const double *__restrict__ Tm, const int *__restrict__ tab, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<FcElem, QT>];
    WG_PROLOGUE(false);
    const double *Tb = Tm + (size_t)T.b * T.ld * T.ld, *Qm = L.Kmat + (size_t)T.b * T.ld * T.ld;
    const FcTab F = fc_tab(tab, T.b, T.ld);
    const int k0 = 64 * F.c0, k1 = 64 * F.c1;
    const bool tri = T.I == T.J;
    WgAcc acc = fc_phase1(fc_zero_acc(), smem, T, Tb, 64 * T.I, Qm, 64 * T.J, k0, k1, tri, FcNoHook(), FcNoHook());
    acc = fc_phase1(acc, smem, T, Qm, 64 * T.I, Tb, 64 * T.J, k0, k1, tri, FcNoHook(), FcNoHook());
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, FcElem());
}
