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
//   k_basis_small  k_mean_small without the segment table: c and A run over all rows, in the same four-row-class / one-thread-per-
//                  element fixed orders; the improper entry is the failed pivot of A alone (flat-prior columns that are linearly
//                  dependent on the patient's rows): status -1.  A pivot fails when it is not above basis_pivot_tol(p) = 4 p 2^-52
//                  times the column's own diagonal entry of A: what rounding can leave of an EXACTLY dependent column, whose
//                  pivot is noise of either sign (a plain "pivot <= 0" would pass half of them); a zero column's pivot is 0
//   k_mean_panel, k_mean_wgrad (kernels_mean.h), k_slabsum, k_epilogue, k_pjvp_solve: unchanged.  k_mean_panel takes its column count
//                  from the view's D, so it is handed a view whose D is p; k_mean_wgrad its k range as an argument
//   k_basis_post   k_mean_post with the tile's rows of h2 (the caller's point order) where that one has e_{m*_j}
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

// ------------------------------------------------------------------------------------------
// grid = the class's entries.  in = [b0 | lam] of the CALL in the caller's entry order (nbatch_call rows of p each), wvec and small:
// the class's part of the call's buffers (mean_tables.h with p columns).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basis_small(MedgpDev L, const double *__restrict__ G, const double *__restrict__ in, int nbatch_call,
                                                     int mode, int p, double *__restrict__ wvec, double *__restrict__ small) {
    constexpr int TRI = BASIS_MAX_P * (BASIS_MAX_P + 1) / 2;
    __shared__ double Ap[TRI], Tp[TRI];
    __shared__ double s_b0[BASIS_MAX_P], s_lam[BASIS_MAX_P], s_c[BASIS_MAX_P], s_u[BASIS_MAX_P], s_dl[BASIS_MAX_P], s_d0[BASIS_MAX_P];
    __shared__ double red[256];
    __shared__ int s_fail;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (L.status[b] < 0) return;
    const int slot = L.bslot[b], n = L.pn[slot], ld = L.ldn, npad = medgp_roundup(n, 64);
    const int pos = L.bpos ? L.bpos[b] : b;   // the caller's row of this entry
    const bool marginal = mode == MEDGP_MEAN_MARGINAL;
    const double *z = L.z + (size_t)b * ld;
    double *wv = wvec + mean_vec_at(b, ld, 0);
    double *sm = small + (size_t)b * mean_small_stride(p);
    for (int d = tid; d < p; d += 256) {
        s_b0[d] = in[(size_t)pos * p + d];
        s_lam[d] = marginal ? in[(size_t)nbatch_call * p + (size_t)pos * p + d] : 0.0;
    }
    if (tid == 0) s_fail = 0;
    __syncthreads();
    // w = z - G b0, columns in order
    for (int i = tid; i < npad; i += 256) {
        double s = 0.0;
        if (i < n) {
            s = z[i];
            for (int d = 0; d < p; d++) s -= G[mean_panel_at(b, ld, i, d)] * s_b0[d];
        }
        wv[i] = s;
    }
    __syncthreads();
    // c = G^T w: four row classes per column, added in a fixed order
    {
        const int d = tid & 63, part = tid >> 6;
        double s = 0.0;
        if (d < p)
            for (int i = part; i < n; i += 4) s += G[mean_panel_at(b, ld, i, d)] * wv[i];
        red[tid] = s;
        __syncthreads();
        if (tid < p) s_c[tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
        __syncthreads();
    }
    double logA = 0.0;   // thread 0: sum log diag chol(A) = 1/2 log|A|
    if (marginal) {
        // A = Lambda + G^T G, lower triangle, one thread per element, rows in order
        for (int idx = tid; idx < p * (p + 1) / 2; idx += 256) {
            int d, e;
            tile_decode(idx, d, e);
            double s = 0.0;
            for (int i = 0; i < n; i++) s += G[mean_panel_at(b, ld, i, d)] * G[mean_panel_at(b, ld, i, e)];
            Ap[mean_tri_at(d, e)] = (d == e) ? s_lam[d] + s : s;
            if (d == e) s_d0[d] = s_lam[d] + s;
        }
        __syncthreads();
        // right-looking Cholesky in place; a pivot fails when it is NaN or not above basis_pivot_tol(p) A_jj (0 for a zero column)
        const double tol = basis_pivot_tol(p);
        for (int j = 0; j < p; j++) {
            if (tid == 0) {
                const double piv = Ap[mean_tri_at(j, j)];
                if (!(piv > tol * s_d0[j])) s_fail = 1;
                Ap[mean_tri_at(j, j)] = sqrt(piv);
            }
            __syncthreads();
            if (s_fail) break;   // (workgroup-uniform: read behind the barrier)
            const double ljj = Ap[mean_tri_at(j, j)];
            for (int i = j + 1 + tid; i < p; i += 256) Ap[mean_tri_at(i, j)] = Ap[mean_tri_at(i, j)] / ljj;
            __syncthreads();
            const int m = p - 1 - j;   // trailing rows j + 1 .. p - 1
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
        if (tid < p) {
            const int j = tid;
            for (int i = j; i < p; i++) {
                double s = (i == j) ? 1.0 : 0.0;
                for (int k = j; k < i; k++) s -= Ap[mean_tri_at(i, k)] * Tp[mean_tri_at(k, j)];
                Tp[mean_tri_at(i, j)] = s / Ap[mean_tri_at(i, i)];
            }
        }
        __syncthreads();
        if (tid < p) {   // u = Ti c
            double s = 0.0;
            for (int e = 0; e <= tid; e++) s += Tp[mean_tri_at(tid, e)] * s_c[e];
            s_u[tid] = s;
        }
        __syncthreads();
        if (tid < p) {   // delta = Ti^T u
            double s = 0.0;
            for (int k = tid; k < p; k++) s += Tp[mean_tri_at(k, tid)] * s_u[k];
            s_dl[tid] = s;
        }
        if (tid == 0)
            for (int d = 0; d < p; d++) logA += log(Ap[mean_tri_at(d, d)]);
        __syncthreads();
    } else {
        for (int d = tid; d < p; d += 256) s_dl[d] = 0.0;
        __syncthreads();
    }
    // the small outputs
    for (int d = tid; d < p; d += 256) {
        sm[mean_off_beta(p) + d] = s_b0[d] + s_dl[d];
        sm[mean_off_dmean(p) + d] = marginal ? -(s_lam[d] * s_dl[d]) : -s_c[d];
        sm[mean_off_delta(p) + d] = s_dl[d];
    }
    for (int idx = tid; idx < p * p; idx += 256) {
        const int d = idx / p, e = idx - d * p;
        double ti = 0.0, cv = 0.0;
        if (marginal) {
            if (e <= d) ti = Tp[mean_tri_at(d, e)];
            for (int k = max(d, e); k < p; k++) cv += Tp[mean_tri_at(k, d)] * Tp[mean_tri_at(k, e)];   // A^-1 = Ti^T Ti
        }
        sm[mean_off_ti(p) + idx] = ti;
        sm[mean_off_cov(p) + idx] = cv;
    }
    // quad = |w - G delta|^2 + sum lam delta^2: per thread the rows tid, tid + 256, ... in order, then one fixed tree
    {
        double s = 0.0;
        for (int i = tid; i < n; i += 256) {
            double r = wv[i];
            if (marginal)
                for (int d = 0; d < p; d++) r -= G[mean_panel_at(b, ld, i, d)] * s_dl[d];
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
            for (int d = 0; d < p; d++) {
                quad += s_lam[d] * (s_dl[d] * s_dl[d]);
                if (s_lam[d] > 0.0) loglam += log(s_lam[d]);
                else nfree++;
            }
        // (scal[0] = sum log diag L = 1/2 log|K|, as k_epilogue reads it)
        L.scal[b * 4 + 2] = quad / 2.0 + L.scal[b * 4 + 0] + logA - loglam / 2.0 + (n - nfree) * log(2. * L.pi) / 2.0;
    }
}

// ------------------------------------------------------------------------------------------
// grid = the chunk's tiles (k_pjvp_solve of the same chunk left V behind the first panel of every tile's work rows).  Wave w owns the
// rows c = 16 w .. of the p x 64 tile G^T V; h2: [M][p], mean / var: fp64, all in the call's point order.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basis_post(MedgpDev L, const PostTile *__restrict__ tiles, const int *__restrict__ meta2,
                                                    const double *__restrict__ h2, const double *__restrict__ work, size_t work_stride,
                                                    const double *__restrict__ G, const double *__restrict__ small, int mode, int p,
                                                    double *__restrict__ mean, double *__restrict__ var) {
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
    const double *sm = small + (size_t)b * mean_small_stride(p);
    v4d acc[4];
#pragma unroll
    for (int cs = 0; cs < 4; cs++) acc[cs] = (v4d){0.0, 0.0, 0.0, 0.0};
    if (16 * w < p)   // wave-uniform
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
        const double *hrow = h2 + pt * (size_t)p;
        const double mean0 = ((part[0][0][tid] + part[0][1][tid]) + part[0][2][tid]) + part[0][3][tid];
        const double vv = ((part[1][0][tid] + part[1][1][tid]) + part[1][2][tid]) + part[1][3][tid];
        double kss = 0.0;
        for (int q = 0; q < Q; q++) kss += B[(size_t)q * D * D + m2 * D + m2];
        const double var0 = (kss - vv) + hyp[m2];
        double dm = 0.0, extra = 0.0;
        for (int d = 0; d < p; d++) dm += (hrow[d] - Cs[d][tid]) * sm[mean_off_beta(p) + d];
        if (mode == MEDGP_MEAN_MARGINAL)
            for (int k = 0; k < p; k++) {
                double u = 0.0;
                for (int e = 0; e <= k; e++) u += sm[mean_off_ti(p) + (size_t)k * p + e] * (hrow[e] - Cs[e][tid]);
                extra += u * u;
            }
        mean[pt] = mean0 + dm;
        var[pt] = var0 + extra;
    }
}
