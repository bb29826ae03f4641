// kernels_posterior_vjp.h -- the reverse mode of kernels_posterior_jvp.h (medgp_posterior_vjp_batch): for cotangents cm_j, cv_j of the
// posterior mean and variance at the test points of an entry, the gradient  sum_j cm_j dmean_j/dtheta + cv_j dvar_j/dtheta  over all
// hypers from ONE weighted gradient pass.  Works behind one pipeline run (L, U = L^-T, z = L^-1 y, alpha) and the unchanged
// k_pjvp_solve, which left W = P K* (work rows, first panel) and V = L^-1 K* (second panel) of every tile of the launch chunk.  With
//   c = W cm (N),   Wc = W diag(cv) (N x m)
// the adjoint of the JVP's formulas (dmean = kdot*^T alpha - w^T Kdot alpha,  dvar = kdot** + sigdot - 2 kdot*^T w + w^T Kdot w) is
//   train-train  1/2 tr(G dK/dtheta_h),        G = 2 Wc W^T - (c alpha^T + alpha c^T)   (symmetric; diag(G) feeds the noise lines)
//   train-test   sum_ij R_ij dk*_ij/dtheta_h,   R = alpha cm^T - 2 Wc                     (no noise term)
//   test diag    sum_j cv_j (sum_q dB_q[m_j,m_j]/dtheta_h + 2 sigma^2_{m_j} [h = sigma_{m_j}])
// The definition is tests/posterior_vjp_truth.py (the reference has no such output).
//
// The convention of the block sums (read from wg_phase3, k_slabsum and k_epilogue): k_slabsum leaves the LOWER bins d >= e,
//   S_q[d,e] = sum_{i in d, j in e} G_ij k_q(t_i - t_j)   (all pairs of the two covariates; d = e: the full square, both triangles),
// and k_epilogue evaluates  1/2 sum_{d,e} dB_q[d,e] Sfull_q[d,e]  with Sfull the symmetric completion (sym_get; the mu / v lines weigh
// d > e twice).  The rectangular sums X_q[d,e] = sum_{i in d, test j in e} R_ij k_q(t_i - t*_j) are NOT symmetric and carry no 1/2;
// dB_q is symmetric, so they enter as  S_q[d,e] += X_q[d,e] + X_q[e,d]  (d > e)  and  S_q[d,d] += 2 X_q[d,d].  The test diagonal adds
// 2 sum_{j: m_j = d} cv_j to S_q[d,d] of every q (k_q(0) = 1; nothing to SM, SV) and to the noise sum of d.  The same holds for SM
// (element -(w_q dt) sin(w_q dt) E_q) and SV (-2 c_q dt^2 k_q), dt = t_i - t*_j.
//
//   k_pvjp_cot    per entry: the fp64 plug-in mean_j = V_j^T z and var_j = k** - V_j^T V_j + sigma^2 (the float outputs stay
//                 k_pjvp_solve's), the cotangents (custom: the caller's; built-in: from mean, var, y, wt), the entry's loss in the
//                 CALLER's point order, c = W cm, the per-covariate sums of cv and the cos / sin tables of the points
//   k_pvjp_wgrad  k_wgrad's prologue and phases 2, 3 behind a phase 1 that forms  sum_k W[I rows][k] cv_k W[J rows][k]  over the entry's
//                 point tiles on fp64 MFMA (row stride 64; cv by a hook on the staged operand, zero beyond the tile's count); tile element
//                 2 ws - (c_i alpha_j + alpha_i c_j); diag(G) leaves through wdiag as in k_wgrad.  G never reaches HBM.
//   k_slabsum     (kernels_core.h, unchanged)
//   k_pvjp_cross  one wave per lower bin (d, e): X_q[d,e] and X_q[e,d], lanes stride over the (row, point) pairs of the bin in a fixed
//                 order, one fixed butterfly; folds them and the test diagonal into S, SM, SV behind k_slabsum
//   k_epilogue    (kernels_core.h, unchanged; epi_mode = EPI_BARE: gradient lines alone, no prior, no scalar)
//   k_pvjp_finish adds the test diagonal's noise term  sigma_d^2 2 sum cv  to line d (a covariate with test points and no observation
//                 has no row in wdiag) and turns the lines of an entry whose built-in loss is NaN into NaN
// The host sorts every patient's points by covariate (stable) before the upload (pvjp_tables.h), so the points of a covariate are a
// range.  No atomics, every sum in a fixed order over operands of the entry and the cotangent set alone: an entry's bits depend
// neither on its batch-mates, nor on the number of cotangent sets or the set's position, nor on the launch chunk.  They DO depend on
// the order of the points inside one covariate (the pair order of k_pvjp_cross, the k order of the MFMA product).
#pragma once
#include "kernels_posterior_jvp.h"
#include "kernels_forecast_grad.h"
#include "pvjp_tables.h"

// ------------------------------------------------------------------------------------------
// grid = the chunk's entries; L: the view of the chunk's first entry.  pin = [cot_mean ncot M | cot_var ncot M | y2 M | wt M] in the
// device's point order (the last two: built-in kinds), pts = [cm M | cv M | l M | cos Q M | sin Q M | mean M | var M] (the last two: the fp64
// plug-in posterior, read back by medgp_posterior_vjp_moments), small = per entry
// [sum cv D | loss | -]; dev_of[caller point] = device point.  Four row classes per column (rows i = w mod 4), added in a fixed order.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pvjp_cot(MedgpDev L, const PvjpEnt *__restrict__ ents, const int *__restrict__ meta2,
                                                  const double *__restrict__ t2, const int *__restrict__ dev_of,
                                                  const double *__restrict__ work, size_t work_stride, const double *__restrict__ pin,
                                                  double *__restrict__ pts, double *__restrict__ cvec, double *__restrict__ small,
                                                  size_t Mz, int kind, int ncot, int set, int has_wt) {
    __shared__ double part[2][4][64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const PvjpEnt E = ents[b];
    const int D = L.D, Q = L.Q;
    double *sm = small + (size_t)b * (D + 2);
    double *mean64 = pts + (3 + 2 * (size_t)Q) * Mz, *var64 = mean64 + Mz;
    if (L.status[b] < 0) {
        if (tid == 0) sm[D] = __builtin_nan("");
        for (int j = tid; j < E.m; j += 256) { mean64[(size_t)E.p0 + j] = __builtin_nan(""); var64[(size_t)E.p0 + j] = __builtin_nan(""); }
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L);
    const double *z = L.z + (size_t)b * ld;
    double *cm = pts, *cv = pts + Mz, *lt = pts + 2 * Mz, *pcs = pts + 3 * Mz, *psn = pcs + (size_t)Q * Mz;
    const double *in_cm = pin + (size_t)set * Mz, *in_cv = pin + ((size_t)ncot + set) * Mz;
    const double *y2 = pin + 2 * (size_t)ncot * Mz, *wt = y2 + Mz;
    const int ntile = (E.m + 63) / 64;
    for (int tt = 0; tt < ntile; tt++) {
        const double *Vf = work + (size_t)(E.tile0 + tt) * work_stride + (size_t)ld * 64;
        const int cnt = min(64, E.m - 64 * tt);
        double s1 = 0.0, s2 = 0.0;
        if (lane < cnt)
            for (int i = w; i < n; i += 4) {
                const double v = Vf[(size_t)i * 64 + lane];
                s1 += v * z[i];
                s2 += v * v;
            }
        __syncthreads();   // (the previous tile's sums are taken)
        part[0][w][lane] = s1;
        part[1][w][lane] = s2;
        __syncthreads();
        if (tid < cnt) {
            const size_t p = (size_t)E.p0 + 64 * tt + tid;
            const int m2 = meta2[p];
            const double mean = ((part[0][0][tid] + part[0][1][tid]) + part[0][2][tid]) + part[0][3][tid];
            const double vv = ((part[1][0][tid] + part[1][1][tid]) + part[1][2][tid]) + part[1][3][tid];
            double kss = 0.0;
            for (int q = 0; q < Q; q++) kss += B[(size_t)q * D * D + m2 * D + m2];
            const double var = (kss - vv) + hyp[m2];
            double a = 0.0, c = 0.0, l = 0.0;
            if (kind == MEDGP_PLOSS_CUSTOM) {
                a = in_cm[p];
                c = in_cv[p];
            } else {
                const double wj = has_wt ? wt[p] : 1.0, r = y2[p] - mean;
                if (kind == MEDGP_PLOSS_SQERR) {
                    l = r * r;
                    a = -2.0 * r;
                } else if (!(var > 0.0)) {
                    l = a = c = __builtin_nan("");
                } else if (kind == MEDGP_PLOSS_NLPD) {
                    l = 0.5 * log(6.283185307179586476925 * var) + (r * r) / (2.0 * var);
                    a = -r / var;
                    c = 0.5 / var - (r * r) / (2.0 * var * var);
                } else {   // CRPS of a normal forecast
                    const double s = sqrt(var), zz = r / s;
                    const double phi = 0.3989422804014326779399 * exp(-0.5 * zz * zz), e2 = erf(zz * 0.7071067811865475244008);   // 2 Phi(z) - 1
                    l = s * (zz * e2 + 2.0 * phi - 0.5641895835477562869481);
                    a = -e2;
                    c = (2.0 * phi - 0.5641895835477562869481) / (2.0 * s);
                }
                l *= wj; a *= wj; c *= wj;
            }
            cm[p] = a;
            cv[p] = c;
            lt[p] = l;
            mean64[p] = mean;
            var64[p] = var;
        }
    }
    // the points' tables (any order: one value each)
    for (int x = tid; x < E.m * Q; x += 256) {
        const int q = x / E.m, j = x - q * E.m;
        double sn, cs;
        sincos(wq[q] * t2[(size_t)E.p0 + j], &sn, &cs);
        pcs[(size_t)q * Mz + E.p0 + j] = cs;
        psn[(size_t)q * Mz + E.p0 + j] = sn;
    }
    __syncthreads();   // cm, cv, lt of the entry are written (global memory, this workgroup)
    // c_i = sum_j W_ij cm_j, points in order
    for (int i = tid; i < npad; i += 256) {
        double s = 0.0;
        if (i < n)
            for (int j = 0; j < E.m; j++) s += work[(size_t)(E.tile0 + (j >> 6)) * work_stride + (size_t)i * 64 + (j & 63)] * cm[(size_t)E.p0 + j];
        cvec[(size_t)b * ld + i] = s;
    }
    // per covariate: sum of cv over its points, in order (the points are sorted by covariate: E.p0 + seg[d] .. seg[d + 1])
    for (int d = tid; d < D; d += 256) {
        double s = 0.0;
        for (int j = 0; j < E.m; j++) s += (meta2[(size_t)E.p0 + j] == d) ? cv[(size_t)E.p0 + j] : 0.0;
        sm[d] = s;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < E.m; j++) s += lt[dev_of[(size_t)E.p0 + j]];
        sm[D] = s;
    }
}

// cv on the staged operand: columns of the tile beyond its count are zero
struct PvCvHook {
    const double *cv;   // of the tile's first point
    int cnt;
    __device__ __forceinline__ v2d operator()(v2d x, int, int col) const {
        x[0] *= (col < cnt) ? cv[col] : 0.0;
        x[1] *= (col + 1 < cnt) ? cv[col + 1] : 0.0;
        return x;
    }
};

// fc_phase1 (kernels_forecast_grad.h) for operands with a row stride of 64 doubles -- the work rows of one point tile: acc += A[rowa0 ..
// + 64][k] B[rowb0 .. + 64][k] over the columns 0 <= k < k1 (a multiple of WG_KC, at most 64).  Ends behind a barrier.
template <class HookB>
__device__ __forceinline__ WgAcc pv_phase1(const WgAcc in, double *smem, const WgTile T, const double *A, int rowa0, const double *B, int rowb0,
                                           int k1, bool tri, const HookB hb) {
    double (*Bs)[64][WG_KC + 2] = (double (*)[64][WG_KC + 2])smem;   // Bs[2][64][34]
    v4d acc[4];
#pragma unroll
    for (int ct = 0; ct < 4; ct++) acc[ct] = in.a[ct];
    const int nch = k1 / WG_KC;   // workgroup-uniform
    if (nch > 0) {
        const int ctmax = tri ? T.w : 3;   // wave-uniform
        const int li = T.li, g = T.g;
        const int srow = T.tid >> 2, scg = (T.tid & 3) * 8;
        const int arow = rowa0 + 16 * T.w + li, brow = rowb0 + srow;
        const double *Arow = A + (size_t)arow * 64 + 2 * g;
        const double *Bsrc = B + (size_t)brow * 64 + scg;
        v2d bst[4], an[4];
#pragma unroll
        for (int u = 0; u < 4; u++) bst[u] = hb(*(const v2d *)(Bsrc + 2 * u), brow, scg + 2 * u);
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
                const int kc = (c + 1) * WG_KC;
#pragma unroll
                for (int u = 0; u < 4; u++) bst[u] = hb(*(const v2d *)(Bsrc + kc + 2 * u), brow, kc + scg + 2 * u);
#pragma unroll
                for (int h = 0; h < 4; h++) an[h] = *(const v2d *)(Arow + kc + 8 * h);
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

// phase-3 element: G_ij = 2 ws_ij - (c_i alpha_j + alpha_i c_j)
struct PvElem {
    static constexpr int NX = 1;
    const double *c;   // of the entry
    __device__ __forceinline__ double extra(int k) const { return c[k]; }
    __device__ __forceinline__ double elem(double ws, double ai, double aj, double ci, double cj) const { return 2.0 * ws - (ci * aj + ai * cj); }
};

// ------------------------------------------------------------------------------------------
// G tile + gradient block reductions of a chunk's entries (L: the view of the chunk's first entry).  The k range of the product is the
// entry's points, tile by tile, each rounded up to WG_KC columns (W is zero beyond the count, cv is taken as zero there).  An entry
// without points: G = 0.  QT / Q0 as in k_wgrad: 8 < Q <= 16 takes two launches, each forming the tile again.
// ------------------------------------------------------------------------------------------
// (workgroups per SIMD promised to the compiler: at k_wgrad's three the instantiation <8> does not fit 168 VGPRs and spills, as k_wgrad<8>
// itself does; two leave it 256 -- kernels_hess.h's rule)
constexpr int pvjp_wgrad_minwaves(int QT) { return QT >= 8 ? 2 : WG_MINWAVES; }
template <int QT, int Q0 = 0>
__global__ void __launch_bounds__(WG_THREADS, pvjp_wgrad_minwaves(QT)) k_pvjp_wgrad(MedgpDev L, const PvjpEnt *__restrict__ ents, const double *__restrict__ work,
                                                                         size_t work_stride, const double *__restrict__ cv,
                                                                         const double *__restrict__ cvec, int nbatch, int ntiles, int nbp) {
    __shared__ __attribute__((aligned(16))) double smem[WG_SMEM_DOUBLES];
    __shared__ __attribute__((aligned(16))) double rowc[4][16][wg_rowc_stride<PvElem, QT>];
    WG_PROLOGUE(false);
    const PvjpEnt E = ents[T.b];
    const bool tri = T.I == T.J;
    const int m = __builtin_amdgcn_readfirstlane(E.m), tile0 = __builtin_amdgcn_readfirstlane(E.tile0), p0 = __builtin_amdgcn_readfirstlane(E.p0);
    WgAcc acc = fc_zero_acc();
    for (int tt = 0; 64 * tt < m; tt++) {
        const double *Wk = work + (size_t)(tile0 + tt) * work_stride;
        const int cnt = min(64, m - 64 * tt);
        acc = pv_phase1(acc, smem, T, Wk, 64 * T.I, Wk, 64 * T.J, medgp_roundup(cnt, WG_KC), tri, PvCvHook{cv + p0 + 64 * tt, cnt});
    }
    wg_phase2(acc, smem, T);
    wg_phase3<QT, Q0>(L, T, smem, rowc, PvElem{cvec + (size_t)T.b * T.ld});
}

// The sums of one (row covariate dr, point covariate de) bin for component q over this wave's lanes: pairs p = lane, lane + 64, ...,
// pair p = (row r0 + p / npt, point c0 + p % npt), then one butterfly.  Returns (sum R e cd, sum R e sd dt, sum R e cd dt^2).
struct PvSums { double s, m, v; };
__device__ __forceinline__ PvSums pv_bin(const MedgpDev &L, const PvjpEnt E, int b, int lane, int q, int r0, int r1, int c0, int c1,
                                         const double *__restrict__ t, const double *__restrict__ al, const double *__restrict__ t2,
                                         const double *__restrict__ cm, const double *__restrict__ cv, const double *__restrict__ pcs,
                                         const double *__restrict__ psn, const double *__restrict__ work, size_t work_stride, double c2n) {
    const int ld = L.ldn, npt = c1 - c0, np = (r1 - r0) * npt;
    const double *csb = L.cs + ((size_t)b * L.Q + q) * ld, *snb = L.sn + ((size_t)b * L.Q + q) * ld;
    double aS = 0.0, aM = 0.0, aV = 0.0;
    for (int p = lane; p < np; p += 64) {
        const int ri = p / npt, i = r0 + ri, jl = c0 + (p - ri * npt);
        const size_t pj = (size_t)E.p0 + jl;
        const double wij = work[(size_t)(E.tile0 + (jl >> 6)) * work_stride + (size_t)i * 64 + (jl & 63)];
        const double r = al[i] * cm[pj] - 2.0 * (wij * cv[pj]);
        const double dt = t[i] - t2[pj], dd = dt * dt;
        const double rc = csb[i], rs = snb[i], cc = pcs[pj], sn = psn[pj];
        const double cd = rc * cc + rs * sn, sd = rs * cc - rc * sn;
        const double re = r * exp2_nonpos(c2n * dd);
        const double pr = re * cd;
        aS += pr;
        aM += (re * sd) * dt;
        aV += pr * dd;
    }
    for (int off = 32; off > 0; off >>= 1) { aS += __shfl_xor(aS, off); aM += __shfl_xor(aM, off); aV += __shfl_xor(aV, off); }
    return PvSums{aS, aM, aV};
}

// ------------------------------------------------------------------------------------------
// Rectangular block sums and the fold into S, SM, SV (behind k_slabsum).  grid = (ceil(D (D + 1) / 2 / 4), the chunk's entries), wave w
// of a workgroup owns the lower bin 4 blockIdx.x + w.  pseg: [entry][D + 1] the points' covariate ranges (relative to the entry's
// first point).  pts as in k_pvjp_cot, its cos / sin tables with stride Mz.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pvjp_cross(MedgpDev L, const PvjpEnt *__restrict__ ents, const int *__restrict__ pseg,
                                                    const double *__restrict__ t2, const double *__restrict__ work, size_t work_stride,
                                                    const double *__restrict__ pts, const double *__restrict__ small, size_t Mz) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int D = L.D, Q = L.Q;
    const int bin = 4 * (int)blockIdx.x + (int)(threadIdx.x >> 6);
    if (bin >= D * (D + 1) / 2 || L.status[b] < 0) return;
    int d, e;
    tile_decode(bin, d, e);
    const PvjpEnt E = ents[b];
    const int slot = L.bslot[b];
    const int *seg = L.pseg + (size_t)slot * (D + 1), *ps = pseg + (size_t)E.ent * (D + 1);
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *t = L.pt + (size_t)slot * L.pld, *al = L.alpha + (size_t)b * L.ldn;
    const double *cm = pts, *cv = pts + Mz, *pcs = pts + 3 * Mz, *psn = pcs + (size_t)Q * Mz;
    const double diag = (d == e) ? 2.0 * small[(size_t)b * (D + 2) + d] : 0.0;
    double *S = L.S + (size_t)b * Q * D * D, *SM = L.SM + (size_t)b * Q * D * D, *SV = L.SV + (size_t)b * Q * D * D;
    for (int q = 0; q < Q; q++) {
        const double wq = hyp[hyp_off_w(L) + q], cq = hyp[hyp_off_c(L) + q], c2n = -cq * MEDGP_LOG2E;
        const PvSums x = pv_bin(L, E, b, lane, q, seg[d], seg[d + 1], ps[e], ps[e + 1], t, al, t2, cm, cv, pcs + (size_t)q * Mz, psn + (size_t)q * Mz, work, work_stride, c2n);
        PvSums y = x;
        if (d != e) y = pv_bin(L, E, b, lane, q, seg[e], seg[e + 1], ps[d], ps[d + 1], t, al, t2, cm, cv, pcs + (size_t)q * Mz, psn + (size_t)q * Mz, work, work_stride, c2n);
        if (lane == 0) {
            const size_t at = (size_t)q * D * D + d * D + e;
            S[at] = S[at] + ((x.s + y.s) + diag);
            SM[at] = SM[at] + (-wq) * (x.m + y.m);
            SV[at] = SV[at] + (-2.0 * cq) * (x.v + y.v);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Behind k_epilogue: line d (a noise line) += sigma_d^2 2 sum_{j: m_j = d} cv_j; an entry whose loss is NaN (a non-positive variance
// under NLPD / CRPS) gets NaN on every line.  grad: the rows k_epilogue wrote (same base pointer, same row rule).  grid = the entries.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pvjp_finish(MedgpDev L, const double *__restrict__ small, double *__restrict__ grad, int builtin) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (L.status[b] < 0) return;   // (k_epilogue wrote the NaNs)
    const int D = L.D, H = L.H;
    const double *sm = small + (size_t)b * (D + 2), *hyp = L.hyp + (size_t)b * L.hyp_stride;
    double *g = grad + (size_t)(L.bpos ? L.bpos[b] : b) * H;
    const double loss = sm[D];
    if (builtin && loss != loss) {
        for (int h = tid; h < H; h += 256) g[h] = __builtin_nan("");
        return;
    }
    for (int d = tid; d < L.nlik; d += 256) g[d] = g[d] + hyp[d] * (2.0 * sm[d]);
}
