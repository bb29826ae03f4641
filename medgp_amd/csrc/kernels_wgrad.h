// kernels_wgrad.h -- fused  W = K^-1 - alpha alpha^T  (never written to HBM) + gradient block reductions.
//
// Replaces the reference's  Q = L^-T L^-1 - alpha alpha^T  (two sgemm, ref: inference/c_inference_exact.cpp:168-172)
// and the per-hyper loop of c_kernel_LMC_SM::compute_self_gradients (ref: kernel/c_kernel_LMC_SM.cpp:198-327),
// regrouped into block sums:
//     S_q [d,e] = sum_{i in d, j in e} W_ij k_q(t_i - t_j)
//     SM_q[d,e] = sum W_ij * ( -(w_q dt) sin(w_q dt) E_q )         (d k_q / d log mu_q,  ref :379-384)
//     SV_q[d,e] = sum W_ij * ( -2 c_q dt^2 k_q )                   (d k_q / d log v_q,   ref :385-391)
// One workgroup (4 waves) per lower 64x64 tile (I, J) of one patient:
//   phase 1  W tile = U[I rows] U[J rows]^T on fp64 MFMA (U = L^-T from k_cholinv; k runs over columns >= 64 I);
//            the J-row fragments are staged through LDS (shared by the 4 waves), the I-row fragments stream
//            from HBM with 16-byte loads.  The first 16 w columns are zero in all of wave w's rows (U is upper
//            triangular): their MFMAs are not issued (WG_MFMA_SKIP_HALVES / _CHUNKS), same bits.
//   phase 2  tile -> LDS (aliases the staging buffers).
//   phase 3  lane = column j, wave = 16-row group: per element one fp64 exp per mixture component (cos/sin of the
//            time difference come from the per-observation tables by the angle-difference identity).
//            Observations are grouped by output, so the output of the row changes rarely: running sums are
//            flushed at each change and reduced over the column segments in a FIXED order -> bitwise
//            reproducible; every (16-row piece of d) x (column tile piece of e) owns one slab entry, written
//            exactly once (no atomics).  k_epilogue adds the pieces in fixed order.
// The pieces (wg_tile_of, the macro WG_PROLOGUE, wg_phase1, wg_phase2, wg_phase3) are defined once and shared with the LOO kernels of
// kernels_loo_grad.h, which differ by a phase-1 hook and by the tile element alone.  Against the form with the pieces written out in
// its body no instantiation of k_wgrad needs more registers, scratch or LDS, and the counts of MFMA, memory and fp64 instructions are
// the same, but the schedule is not: another instruction stream.  What was measured: profiles/wgrad_shared_resources.txt.
#pragma once
#include "medgp_dev.h"
#include "kernels_assemble.h"

#define WG_KC 32
#define WG_THREADS 256
#ifndef WG_MINWAVES
#define WG_MINWAVES 3
#endif
// staging buffers Bs[2][64][WG_KC + 2] (phase 1) and the W tile Ws[64][66] (phases 2 and 3; 4224 <= 4352 doubles) share storage
#define WG_SMEM_DOUBLES (2 * 64 * (WG_KC + 2))

// what a workgroup knows about its tile: entry b (patient slot `slot`, n observations, npad = n rounded up to 64-blocks), tile (I, J), I >= J
struct WgTile { int b, slot, n, ld, npad, I, J, tid, lane, li, g, w; };

// 1-D grid of 8 * ceil(nbatch / 8) * ntiles workgroups, dealt round-robin over the 8 XCDs by the hardware.
// id -> (patient, tile) keeps a patient on ONE XCD (its U rows are re-read by every tile: they must share an L2) and
// makes the tiles of a patient consecutive in dispatch order, so that an XCD works on about three patients at a time
// (3 x 1.2 MB of U fits its 4 MB L2).  Patient-major over the whole batch instead (all patients' tile 0, then tile
// 1, ...) cycles 64 patients x 1.2 MB through each L2 between two tiles of the same patient: every tile re-read U
// from HBM (PMC: 3.6 GB fetched per launch for 0.6 GB of U).
// With fewer than 64 patients that would leave XCDs idle (one patient = one XCD): spread instead, patient index
// fastest (tiles of a patient then land on XCD b % 8 only when nbatch is a multiple of 8, which no longer matters).
// nbp (launches of fewer than 64 entries): stride of the entry index in the workgroup id, nbatch or nbatch | 1.  Workgroup ids go round-robin
// over the 8 XCDs, so with the entry index fastest entry b's tiles land on 8 / gcd(stride, 8) ... of them: harmless when all entries are
// equally large (every XCD gets the same work: 4 x N = 2048 0.062 ms per entry, 5 x 0.062), but in a RAGGED class of 2, 4 or 8 entries
// the largest entry's tiles -- most of the work -- queue on half, a quarter, an eighth of the chip (round 5, scratch/wgrad_ragged.py:
// N = 3595 + 3 x 2400: 1.18 ms, + 4 x 2400: 0.73 ms).  An odd stride puts every entry on all XCDs; the ids of the padding entry exit.
// SERP: a launch of at most 1024 workgroups (all resident at once) deals its tiles in serpentine order (see k_wgrad).
template <bool SERP>
__device__ __forceinline__ bool wg_tile_of(int nbatch, int ntiles, int nbp, int &b, int &tix) {
    if (nbatch >= 64) {
        const int xcd = blockIdx.x & 7, rest = blockIdx.x >> 3;
        b = (rest / ntiles) * 8 + xcd;
        tix = rest % ntiles;
    } else {
        int x = blockIdx.x;
        const int total = nbp * ntiles;
        if (x >= total) return false;
        if (SERP && total <= 1024 && ((x >> 8) & 1)) {   // odd group of 256: reversed
            const int v0 = x & ~255, m = min(256, total - v0);
            x = v0 + (m - 1 - (x & 255));
        }
        b = x % nbp;
        tix = x / nbp;
    }
    return b < nbatch;
}

// The prologue of a kernel with the arguments (MedgpDev L, ..., int nbatch, int ntiles, int nbp): leaves `const WgTile T`, or returns when
// there is nothing to do (a padding id, a failed entry, a tile beyond the entry's own blocks).  A macro so that these are returns of the kernel.
#define WG_PROLOGUE(SERP) \
    int b_, tix_; \
    if (!wg_tile_of<(SERP)>(nbatch, ntiles, nbp, b_, tix_)) return; \
    if (L.status[b_] < 0) return; \
    const int slot_ = __builtin_amdgcn_readfirstlane(L.bslot[b_]); \
    const int n_ = __builtin_amdgcn_readfirstlane(L.pn[slot_]); \
    const int npad_ = medgp_roundup(n_, 64); \
    int I_, J_; \
    tile_decode(tix_, I_, J_); \
    if (I_ >= npad_ / 64) return; \
    const int tid_ = threadIdx.x, lane_ = tid_ & 63; \
    const WgTile T{b_, slot_, n_, L.ldn, npad_, I_, J_, tid_, lane_, lane_ & 15, lane_ >> 4, __builtin_amdgcn_readfirstlane(tid_ >> 6)}

// Phase-1 hooks: applied to a fragment (two adjacent doubles at column `col` of row `row` of M, in chunk c of the k range) between its
// load and its use.  staged: the J rows on their way into LDS; streamed: the I rows.  Values go in and out by value: a local array handed
// to a function by reference is kept as ONE wide vector by the compiler (k_wgrad<5, 0, 1>: 168 VGPRs and 212 bytes of scratch against 120 / 0).
struct WgNoHook {
    __device__ __forceinline__ v2d staged(v2d x, int, int, int) const { return x; }
    __device__ __forceinline__ v2d streamed(v2d x, int, int, int) const { return x; }
};
struct WgAcc { v4d a[4]; };   // a[ct]: rows 16w.. of block I, cols 16ct.. of block J

// one chunk of the MFMA block of phase 1: rows 16w.. (A fragment ac, streamed) x the four column tiles of the staged J rows
#define WG_CHUNK_MFMA(ac, buf) \
    _Pragma("unroll") for (int h = 0; h < 4; h++) \
        _Pragma("unroll") for (int ct = 0; ct < 4; ct++) { \
            if (ct > ctmax) continue;   /* diagonal tile: columns right of this wave's rows are never used */ \
            const v2d bf = *(const v2d *)&Bs[buf][16 * ct + li][8 * h + 2 * g]; \
            _Pragma("unroll") for (int s = 0; s < 2; s++) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[h][s], bf[s], acc[ct], 0, 0, 0); \
        }

// The zero head of the streamed rows.  When M is upper triangular and the k range starts at the tile's own diagonal block (k0 = 64 I),
// row 64 I + 16 w + r is zero left of column 64 I + 16 w: the first 16 w columns of the range are zero in ALL 16 streamed rows of wave
// w.  Their products are exact zeros, and adding +-0 leaves an accumulator that started at +0 as it is, bit for bit (finite operands:
// entries whose factorisation failed never get here), so their MFMAs are not issued at all; nothing else changes (the wave still
// stages, streams and meets the barriers).  Two forms, both wave-uniform scalar branches:
//   WG_MFMA_SKIP_CHUNKS  one guard around the whole block of a chunk: 16 w / WG_KC whole chunks, chunk 0 for the waves 2 and 3
//                        (8 of the 12 zero stretches of 8 columns of a tile).  The diagonal tiles, whose block already has a guard per
//                        column tile (ctmax), and the PF = 2 loop of k_wgrad take it: any second guard inside such a block -- per 8
//                        columns, per half, nested, if / else -- made the compiler keep two copies of the 32 accumulator registers
//                        and copy them inside the loop (k_wgrad<5, 0, 1> at 132 .. 168 VGPRs: three workgroups per CU).
//   WG_MFMA_SKIP_HALVES  the off-diagonal tiles (all four column tiles in use, so no guard per column tile): one guard per 16-column
//                        half of a chunk, all 12 zero stretches (wave 1: the first half of chunk 0, wave 2: chunk 0, wave 3: chunk 0
//                        and the first half of chunk 1).  k_wgrad<5, 0, 1>: 128 VGPRs, no scratch, four workgroups per CU as before --
//                        but with the guards' test written in columns (16 w - 32 c <= 0 / <= 16) the same loop took 156.
// Registers of every form that was tried, and the ones to re-check after an edit here: profiles/wgrad_zero_work_resources.txt;
// timings: profiles/wgrad_zero_work_timing.txt; the bits: tests/test_wgrad_zero_work_gpu.py.
__device__ __forceinline__ int wg_zero_chunks(int w) { return 16 * w / WG_KC; }
#define WG_MFMA_PLAIN(ac, buf, c) WG_CHUNK_MFMA(ac, buf)
#define WG_MFMA_SKIP_CHUNKS(ac, buf, c) if ((c) >= wg_zero_chunks(T.w)) { WG_CHUNK_MFMA(ac, buf) }
#define WG_HALF_MFMA(ac, buf, h0) \
    _Pragma("unroll") for (int h = (h0); h < (h0) + 2; h++) \
        _Pragma("unroll") for (int ct = 0; ct < 4; ct++) { \
            const v2d bf = *(const v2d *)&Bs[buf][16 * ct + li][8 * h + 2 * g]; \
            _Pragma("unroll") for (int s = 0; s < 2; s++) acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[h][s], bf[s], acc[ct], 0, 0, 0); \
        }
#define WG_MFMA_SKIP_HALVES(ac, buf, c) \
    { \
        const int zs_ = 2 * T.w - (WG_KC / 8) * (c);   /* zero stretches of 8 columns left at the head of this chunk */ \
        if (zs_ <= 0) { WG_HALF_MFMA(ac, buf, 0) } \
        if (zs_ <= 2) { WG_HALF_MFMA(ac, buf, 2) } \
    }

// the chunk loop of wg_phase1, MFMA_BLOCK(ac, buf, c) = one of the three forms above
#define WG_PHASE1_LOOP(MFMA_BLOCK) \
    for (int c = 0; c < nch; c++) { \
        const int buf = c & 1; \
        v2d ac[4]; \
        _Pragma("unroll") for (int h = 0; h < 4; h++) ac[h] = an[h]; \
        if (c + 1 < nch) { \
            const int kc = (c + 1) * WG_KC; \
            _Pragma("unroll") for (int u = 0; u < 4; u++) bst[u] = hk.staged(*(const v2d *)(Bsrc + kc + 2 * u), c + 1, brow, k0 + kc + scg + 2 * u); \
            _Pragma("unroll") for (int h = 0; h < 4; h++) an[h] = hk.streamed(*(const v2d *)(Arow + kc + 8 * h), c + 1, arow, k0 + kc + 2 * g + 8 * h); \
        } \
        MFMA_BLOCK(ac, buf, c) \
        if (c + 1 < nch) { \
            _Pragma("unroll") for (int u = 0; u < 4; u++) *(v2d *)&Bs[buf ^ 1][srow][scg + 2 * u] = bst[u]; \
        } \
        __syncthreads(); \
    }

// Phase 1: the tile  sum over the columns k >= k0 of M[I rows][k] M[J rows][k], one chunk of WG_KC columns prefetched ahead.
// UPPER: the caller's promise that M BEHIND THE HOOK is upper triangular with exact zeros below the diagonal of its diagonal blocks and
// that k0 = 64 I; the MFMAs of the streamed rows' zero head are then skipped (above).  A hook that turns a structural zero into
// something else, or another k range (k_loo_wgrad: rows of the full P from column 0), must leave it false: the loop is then the plain one.
template <bool UPPER, class Hook>
__device__ __forceinline__ WgAcc wg_phase1(double *smem, const WgTile T, const double *M, int k0, const Hook hk) {
    double (*Bs)[64][WG_KC + 2] = (double (*)[64][WG_KC + 2])smem;   // Bs[2][64][34]
    v4d acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[ct] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int nch = (T.npad - k0) / WG_KC;
    const int ctmax = (T.I == T.J) ? T.w : 3;   // wave-uniform
    const int li = T.li, g = T.g;
    const int srow = T.tid >> 2, scg = (T.tid & 3) * 8;
    const int arow = 64 * T.I + 16 * T.w + li, brow = 64 * T.J + srow;
    const double *Arow = M + (size_t)arow * T.ld + k0 + 2 * g;
    const double *Bsrc = M + (size_t)brow * T.ld + k0 + scg;
    v2d bst[4], an[4];
#pragma unroll
    for (int u = 0; u < 4; u++) bst[u] = hk.staged(*(const v2d *)(Bsrc + 2 * u), 0, brow, k0 + scg + 2 * u);
#pragma unroll
    for (int h = 0; h < 4; h++) an[h] = hk.streamed(*(const v2d *)(Arow + 8 * h), 0, arow, k0 + 2 * g + 8 * h);
#pragma unroll
    for (int u = 0; u < 4; u++) *(v2d *)&Bs[0][srow][scg + 2 * u] = bst[u];
    __syncthreads();
    if constexpr (!UPPER) {
        WG_PHASE1_LOOP(WG_MFMA_PLAIN)
    } else if (T.I != T.J) {   // workgroup-uniform
        WG_PHASE1_LOOP(WG_MFMA_SKIP_HALVES)
    } else {
        WG_PHASE1_LOOP(WG_MFMA_SKIP_CHUNKS)
    }
    return WgAcc{{acc[0], acc[1], acc[2], acc[3]}};
}

// Phase 2: tile -> LDS (all waves are past the last staging read: the barrier that ends phase 1)
__device__ __forceinline__ void wg_phase2(const WgAcc acc, double *smem, const WgTile T) {
    double (*Ws)[66] = (double (*)[66])smem;   // Ws[64][66]
#pragma unroll
    for (int ct = 0; ct < 4; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) Ws[16 * T.w + 4 * r + T.g][16 * ct + T.li] = acc.a[ct][r];
    __syncthreads();
}

// Phase-3 element policies: the tile element from the accumulated Ws_ij, alpha_i, alpha_j and NX (0 or 1) further constants of the
// row and of the column, which extra(k) loads for observation k (NX = 0: no load).  The nlml gradient: W_ij = (K^-1)_ij - alpha_i alpha_j.
struct WgElemNlml {
    static constexpr int NX = 0;
    __device__ __forceinline__ double extra(int) const { return 0.0; }
    __device__ __forceinline__ double elem(double ws, double ai, double aj, double, double) const { return ws - ai * aj; }
};
// a row of rowc: t, alpha, [extra, -,] (cos, sin) x QT
template <class Elem, int QT> constexpr int wg_rowc_stride = 2 + 2 * Elem::NX + 2 * QT;

// Phase 3 on the tile in Ws; rowc: [4][16][wg_rowc_stride] doubles of LDS, the row constants of each wave's 16 rows.
// QT = mixture components this launch reduces, Q0 = index of the first one.
template <int QT, int Q0, class Elem>
__device__ __forceinline__ void wg_phase3(const MedgpDev &L, const WgTile T, const double *smem, double (*rowc)[16][wg_rowc_stride<Elem, QT>], const Elem el) {
    constexpr int NX = Elem::NX, RC = 2 + 2 * NX;   // RC: where the (cos, sin) pairs of a rowc row start
    const double (*Ws)[66] = (const double (*)[66])smem;
    const int b = T.b, slot = T.slot, n = T.n, ld = T.ld, I = T.I, J = T.J, lane = T.lane, w = T.w;
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
    const double tj = t[j], aj = alpha[j];
    const double xj = el.extra(j);
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
    // row constants of the wave's 16 rows: loaded once (lane r holds row r, lanes >= 16 mirror), instead of 3 + 2Q
    // dependent scalar loads per row iteration
    const int irow = 64 * I + 16 * w + (lane & 15);
    const double r_t = t[irow], r_a = alpha[irow];
    const double r_x = el.extra(irow);
    const int r_m = (irow < n) ? meta[irow] : -1;
    double r_cs[QT], r_sn[QT];
#pragma unroll
    for (int q = 0; q < QT; q++) { r_cs[q] = csb[q * ld + irow]; r_sn[q] = snb[q * ld + irow]; }
    // row constants go through LDS: every lane reads the same address (a broadcast on the LDS pipe, no VALU) where two
    // v_readlane per double cost 2 + 4Q VALU per row (measured: k_wgrad 1.12 -> 1.07 ms, and 17 VGPRs fewer)
    if (lane < 16) {
        rowc[w][lane][0] = r_t; rowc[w][lane][1] = r_a;
        if constexpr (NX) { rowc[w][lane][2] = r_x; rowc[w][lane][3] = 0.0; }
#pragma unroll
        for (int q = 0; q < QT; q++) { rowc[w][lane][RC + 2 * q] = r_cs[q]; rowc[w][lane][RC + 1 + 2 * q] = r_sn[q]; }
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
                // segment ends up with the segment sum.  (A serial per-segment loop here cost as many VALU instructions
                // as the whole pair loop.)  Step-major: one exec-mask region per step covers the adds of all 3 QT values.
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
        const double ti = ta[0], ai = ta[1];
        const double xi = NX ? rowc[w][rr][2] : 0.0;
        double wv = el.elem(Ws[16 * w + rr][lane], ai, aj, xi, xj);
        if (I == J && j == i) L.wdiag[(size_t)b * ld + i] = wv;   // noise gradient needs the diagonal of the tile matrix
        const bool valid = jv && (j <= i);
        wv = valid ? ((mi == mj && j < i) ? 2.0 * wv : wv) : 0.0;
        const double dt = ti - tj, dd = dt * dt;
        // running sums hold  sum w E cd,  sum w E sd dt,  sum w E cd dt^2 ; the constant factors
        // (-w_q, -2 c_q) are applied once per flush -- 3 VALU less per (pair, component)
#pragma unroll
        for (int q = 0; q < QT; q++) {
            const v2d csn = *(const v2d *)&rowc[w][rr][RC + 2 * q];
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

// QT = mixture components this launch reduces, Q0 = index of the first one (Q <= 8: one launch <Q, 0>; 8 < Q <= 16: <8, 0> and
// <Q - 8, 8>, each forming the W tile again -- N^3/3 more MFMA work for a route no BASELINE config takes).
// PF = chunks the phase-1 loop prefetches ahead.  PF = 2 for launches of few large patients (the chip is filled less than four times): a
// workgroup then shares its SIMDs with at most a few others and little hides the latency of its operand stream; measured k_wgrad 0.123 ->
// 0.108 ms (1 x N = 2048), 0.072 -> 0.064 ms (4 x N = 1024), 0.449 -> 0.437 ms (1 x N = 4096), neutral on full launches (which keep PF = 1,
// the round-3 code path); four chunks ahead and a branch-free MFMA block for the off-diagonal tiles were both slower (DESIGN_LOG A.7).  Such a
// launch of at most 1024 workgroups (all resident at once, so placement is static: workgroups x, x + 256, x + 512 share a CU -- traced) also
// deals its tiles in serpentine order, so that the CU holding the longest k range gets the shortest one next.  Scheduling only: same MFMA
// sequence per tile, same bits.
template <int QT, int Q0 = 0, int PF = 1>
__global__ void __launch_bounds__(WG_THREADS, WG_MINWAVES) k_wgrad(MedgpDev L, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<WgElemNlml, QT>];
    WG_PROLOGUE((PF > 1));
    const double *U = L.Linv + (size_t)T.b * T.ld * T.ld;

#ifdef MEDGP_STAMPS
    unsigned long long wst[4] = {0, 0, 0, 0}, wlast;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wlast)::"memory");
#define WSTAMP(k) do { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); wst[k] += t_ - wlast; wlast = t_; } while (0)
#else
#define WSTAMP(k) do {} while (0)
#endif
    WgAcc A;
    if constexpr (PF == 1) A = wg_phase1<true>(smem, T, U, 64 * T.I, WgNoHook());   // k_cholinv / the look-ahead chain zero U's diagonal blocks below the diagonal
    else {
        // PF register sets, set s carries the chunks c = s (mod PF): a set is refilled (chunk c + PF) as soon as its A fragment has been
        // copied out; its staged J rows go to LDS one iteration before they are used (the LDS stays double buffered)
        double (*Bs)[64][WG_KC + 2] = (double (*)[64][WG_KC + 2])smem;
        v4d (&acc)[4] = A.a;
#pragma unroll
        for (int ct = 0; ct < 4; ct++) acc[ct] = (v4d){0.0, 0.0, 0.0, 0.0};
        const int k0 = 64 * T.I, nch = (T.npad - k0) / WG_KC, li = T.li, g = T.g;
        const int ctmax = (T.I == T.J) ? T.w : 3;   // wave-uniform
        const double *Arow = U + (size_t)(64 * T.I + 16 * T.w + li) * T.ld + k0 + 2 * g;
        const int srow = T.tid >> 2, scg = (T.tid & 3) * 8;
        const double *Bsrc = U + (size_t)(64 * T.J + srow) * T.ld + k0 + scg;
        v2d bst[PF][4], an[PF][4];
#pragma unroll
        for (int st = 0; st < PF; st++)
            if (st < nch) {
#pragma unroll
                for (int u = 0; u < 4; u++) bst[st][u] = *(const v2d *)(Bsrc + st * WG_KC + 2 * u);
#pragma unroll
                for (int h = 0; h < 4; h++) an[st][h] = *(const v2d *)(Arow + st * WG_KC + 8 * h);
            }
#pragma unroll
        for (int u = 0; u < 4; u++) *(v2d *)&Bs[0][srow][scg + 2 * u] = bst[0][u];
        __syncthreads();
        for (int c0 = 0; c0 < nch; c0 += PF) {
#pragma unroll
            for (int st = 0; st < PF; st++) {
                const int c = c0 + st;
                if (c >= nch) break;
                v2d ac[4];
#pragma unroll
                for (int h = 0; h < 4; h++) ac[h] = an[st][h];
                if (c + PF < nch) {
#pragma unroll
                    for (int u = 0; u < 4; u++) bst[st][u] = *(const v2d *)(Bsrc + (c + PF) * WG_KC + 2 * u);
#pragma unroll
                    for (int h = 0; h < 4; h++) an[st][h] = *(const v2d *)(Arow + (c + PF) * WG_KC + 8 * h);
                }
                WG_MFMA_SKIP_CHUNKS(ac, (st & 1), c)   // U from its diagonal block on, as wg_phase1<true>
                if (c + 1 < nch) {
#pragma unroll
                    for (int u = 0; u < 4; u++) *(v2d *)&Bs[(st + 1) & 1][srow][scg + 2 * u] = bst[(st + 1) % PF][u];
                }
                __syncthreads();
            }
        }
    }
    WSTAMP(0);
    wg_phase2(A, smem, T);
    WSTAMP(1);
    wg_phase3<QT, Q0>(L, T, smem, rowc, WgElemNlml());
    WSTAMP(2);
#ifdef MEDGP_STAMPS
    if (T.lane == 0 && T.b < 64) {
        unsigned long long *dbg = (unsigned long long *)(L.xk + (size_t)T.b * 64 * 64);
        for (int e = 0; e < 3; e++) atomicAdd(&dbg[e], wst[e]);
        atomicAdd(&dbg[3], 1ull);
    }
#endif
}
