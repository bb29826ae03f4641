// kernels_gmm.h -- the kernel-clustering step: EM for full-covariance Gaussian mixtures, many independent runs per call
// (DESIGN 4.8a).  fp64 throughout, products on v_mfma_f64_16x16x4_f64.
//
// Replaces, from a supplied start, what scikit-learn's GaussianMixture(covariance_type='full') does for the reference's
// run_sklearn_gmm (ref: medgpc/clustering/cluster.py:23-46): the restarts of every K are the RUNS of one call; the selection
// (largest lower bound per K, smallest BIC over K) is host work in medgp_amd/clustering.py.  The definition the kernels are
// held to is tests/gmm_ref.py.
//
// All runs advance together, one EM iteration per round of seven launches:
//   k_gmm_estep   (block of 64 points, component, run)  Y = (X_blk - mu_k) P_k on MFMA, P_k = L_k^-T upper triangular; the row
//                                                        norms of Y give log p_ik.  diff is staged in LDS whole, P_k by 16-column
//                                                        panels; the zero rows below a panel's diagonal tile are not multiplied
//   k_gmm_resp    (block, run)                           logsumexp over the run's K, responsibilities, per-block partial sums of
//                                                        lse and of r_ik (one wave = the block: fixed butterfly)
//   k_gmm_msum    (chunk of blocks, component, run)      partial sum_i r_ik x_i, points in order
//   k_gmm_means   (component, run)                       n_k (block order), mu_k (chunk order), log w_k
//   k_gmm_cov     (chunk, component, run)                (r . diff)^T diff on MFMA into the chunk's d x d slab, lower tiles only
//   k_gmm_factor  (component, run)                       slabs added in chunk order, / n_k, + reg_covar; Cholesky in LDS; P_k and
//                                                        sum log diag L_k; a bad pivot (<= 0 or NaN, LAPACK's rule) flags the component
//   k_gmm_tail    (run)                                  lb = mean lse (block order), change, and the run's status
// A run whose status is set is FROZEN: its workgroups return at once in every later launch, so its parameters are those of the
// iteration that set the flag and the host may look at the flags as rarely as it likes.  Every sum runs in a fixed order over the
// run's own operands, and the geometry (gmm_tables.h) depends on n and d alone: a run's bits do not depend on its call-mates.
//
// Bounds: the point matrix is padded with zero rows to whole blocks and zero columns to dp = 16 ceil(d / 16); means, P and the
// covariances keep zero padding (k_gmm_means writes 0 / n_k there, k_gmm_factor writes zeros), so no load needs a guard.  Padded
// points get responsibility 0 in k_gmm_resp and never reach an output.
#pragma once
#include <hip/hip_runtime.h>
#include "gmm_tables.h"

typedef double gmm_v4d __attribute__((ext_vector_type(4)));   // the accumulator of v_mfma_f64_16x16x4_f64

#define GMM_LDD (MEDGP_GMM_MAX_D + 1)   // LDS row stride (doubles) of a staged block of points / of the covariance
#define GMM_LDP 17                      // ... of a 16-column panel of P

enum { GMM_RUNNING = 0, GMM_CONVERGED = 1, GMM_FAILED = -1 };
enum { GMM_PHASE_INIT = 0, GMM_PHASE_ITER = 1, GMM_PHASE_FINAL = 2 };

struct GmmDev {
    int n, d, dp, nblk, npad, bpc, nchunk, nruns, kmax;
    double tol, reg;
    const double *x;      // [npad, dp]
    const int *k;         // [nruns]
    int *label;           // [nruns, n]: label0, overwritten by assign in the final phase
    double *resp;         // [nruns, kmax, npad]
    double *mu;           // [nruns, kmax, dp]
    double *cov, *P;      // [nruns, kmax, dp, dp]
    double *nk, *logw, *logdet;   // [nruns, kmax]
    int *cfail;           // [nruns, kmax]
    double *blk_nk;       // [nruns, kmax, nblk]
    double *blk_lse;      // [nruns, nblk]
    double *sx;           // [nruns, kmax, nchunk, dp]
    double *slab;         // [nruns, kmax, nchunk, dp, dp]
    double *lb, *prev, *score;    // [nruns]
    int *niter, *status;  // [nruns]
};

// a frozen run does nothing; the final E-step runs for every run that has not failed
__device__ inline bool gmm_skip(const GmmDev &G, int r, int phase) {
    const int st = G.status[r];
    return phase == GMM_PHASE_FINAL ? st == GMM_FAILED : st != GMM_RUNNING;
}

// stage diff = X_blk - mu_k (64 x dp) into LDS; every index is inside the padded buffers
__device__ inline void gmm_stage_diff(const GmmDev &G, double *Ds, int blk, const double *mu, int tid) {
    const double *xb = G.x + (size_t)blk * GMM_BLOCK * G.dp;
    for (int idx = tid; idx < GMM_BLOCK * G.dp; idx += 256) {
        const int row = idx / G.dp, col = idx - row * G.dp;
        Ds[row * GMM_LDD + col] = xb[idx] - mu[col];
    }
}

__global__ void __launch_bounds__(256) k_gmm_estep(GmmDev G, int phase) {
    __shared__ double Ds[GMM_BLOCK * GMM_LDD];
    __shared__ double Ps[MEDGP_GMM_MAX_D * GMM_LDP];
    const int blk = blockIdx.x, k = blockIdx.y, r = blockIdx.z, tid = threadIdx.x;
    if (gmm_skip(G, r, phase) || k >= G.k[r]) return;
    const int dp = G.dp, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const size_t rk = (size_t)r * G.kmax + k;
    const double *P = G.P + rk * dp * dp;
    gmm_stage_diff(G, Ds, blk, G.mu + rk * dp, tid);
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    for (int jt = 0; jt < dp / 16; jt++) {
        const int kend = 16 * (jt + 1);   // P is upper triangular: rows >= kend of this panel are zero
        __syncthreads();
        for (int idx = tid; idx < kend * 16; idx += 256) Ps[(idx >> 4) * GMM_LDP + (idx & 15)] = P[(size_t)(idx >> 4) * dp + 16 * jt + (idx & 15)];
        __syncthreads();
        gmm_v4d acc = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < kend / 4; s++)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ds[(16 * wave + li) * GMM_LDD + 4 * s + g], Ps[(4 * s + g) * GMM_LDP + li], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; q++) sq[q] = fma(acc[q], acc[q], sq[q]);
    }
    // acc register q of lane (li, g) is Y[row g + 4 q][col li]: add over the 16 columns (lanes of equal g), fixed butterfly
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) sq[q] += __shfl_xor(sq[q], m);
    if (li == 0) {
        const double c = G.d * 1.8378770664093453 /* log 2 pi */, ld = G.logdet[rk], lw = G.logw[rk];
#pragma unroll
        for (int q = 0; q < 4; q++)
            G.resp[rk * G.npad + (size_t)blk * GMM_BLOCK + 16 * wave + g + 4 * q] = -0.5 * (c + sq[q]) - ld + lw;
    }
}

// sum over the 64 lanes of the wave, every lane gets it; the order is fixed
__device__ inline double gmm_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// phase INIT: the responsibilities are the one-hot start labels (lse is not formed); FINAL: also assign = first arg max
__global__ void __launch_bounds__(64) k_gmm_resp(GmmDev G, int phase) {
    const int blk = blockIdx.x, r = blockIdx.y, lane = threadIdx.x;
    if (gmm_skip(G, r, phase)) return;
    const int K = G.k[r];
    const int i = blk * GMM_BLOCK + lane;
    const bool valid = i < G.n;
    double *R = G.resp + (size_t)r * G.kmax * G.npad + i;   // component stride npad
    double *bn = G.blk_nk + (size_t)r * G.kmax * G.nblk + blk;
    if (phase == GMM_PHASE_INIT) {
        const int lab = valid ? G.label[(size_t)r * G.n + i] : -1;
        for (int k = 0; k < K; k++) {
            const double rr = lab == k ? 1.0 : 0.0;
            R[(size_t)k * G.npad] = rr;
            const double s = gmm_wave_sum(rr);
            if (lane == 0) bn[(size_t)k * G.nblk] = s;
        }
        return;
    }
    double m = R[0];
    for (int k = 1; k < K; k++) m = fmax(m, R[(size_t)k * G.npad]);
    double se = 0.0;
    for (int k = 0; k < K; k++) se += exp(R[(size_t)k * G.npad] - m);
    const double lse = m + log(se);
    double best = -1.0;
    int arg = 0;
    for (int k = 0; k < K; k++) {
        const double rr = valid ? exp(R[(size_t)k * G.npad] - lse) : 0.0;
        R[(size_t)k * G.npad] = rr;
        if (rr > best) { best = rr; arg = k; }
        const double s = gmm_wave_sum(rr);
        if (lane == 0) bn[(size_t)k * G.nblk] = s;
    }
    const double sl = gmm_wave_sum(valid ? lse : 0.0);
    if (lane == 0) G.blk_lse[(size_t)r * G.nblk + blk] = sl;
    if (phase == GMM_PHASE_FINAL && valid) G.label[(size_t)r * G.n + i] = arg;
}

__global__ void __launch_bounds__(128) k_gmm_msum(GmmDev G) {
    const int c = blockIdx.x, k = blockIdx.y, r = blockIdx.z, j = threadIdx.x;
    if (gmm_skip(G, r, GMM_PHASE_ITER) || k >= G.k[r] || j >= G.dp) return;
    const size_t rk = (size_t)r * G.kmax + k;
    const int i0 = c * G.bpc * GMM_BLOCK;
    const int i1 = min((c + 1) * G.bpc, G.nblk) * GMM_BLOCK;
    const double *R = G.resp + rk * G.npad;
    double s = 0.0;
    for (int i = i0; i < i1; i++) s = fma(R[i], G.x[(size_t)i * G.dp + j], s);
    G.sx[(rk * G.nchunk + c) * G.dp + j] = s;
}

__global__ void __launch_bounds__(128) k_gmm_means(GmmDev G) {
    const int k = blockIdx.x, r = blockIdx.y, j = threadIdx.x;
    if (gmm_skip(G, r, GMM_PHASE_ITER) || k >= G.k[r]) return;
    const size_t rk = (size_t)r * G.kmax + k;
    double nk = 0.0;   // every thread forms the same sum in the same order
    for (int b = 0; b < G.nblk; b++) nk += G.blk_nk[rk * G.nblk + b];
    nk += 10.0 * 2.220446049250313e-16;   // scikit-learn's 10 eps: an empty class keeps a finite mean
    if (j < G.dp) {
        double s = 0.0;
        for (int c = 0; c < G.nchunk; c++) s += G.sx[(rk * G.nchunk + c) * G.dp + j];
        G.mu[rk * G.dp + j] = s / nk;
    }
    if (j == 0) {
        G.nk[rk] = nk;
        G.logw[rk] = log(nk / G.n);
    }
}

__global__ void __launch_bounds__(256) k_gmm_cov(GmmDev G) {
    __shared__ double Ds[GMM_BLOCK * GMM_LDD];
    __shared__ double rs[GMM_BLOCK];
    const int c = blockIdx.x, k = blockIdx.y, r = blockIdx.z, tid = threadIdx.x;
    if (gmm_skip(G, r, GMM_PHASE_ITER) || k >= G.k[r]) return;
    const int dp = G.dp, wave = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const size_t rk = (size_t)r * G.kmax + k;
    const int nt = dp / 16, ntl = nt * (nt + 1) / 2;   // lower tiles: at most 15, so at most 4 per wave
    int ti[4], tj[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int idx = wave + 4 * q;
        int a = 0;
        while ((a + 1) * (a + 2) / 2 <= idx) a++;
        ti[q] = a;
        tj[q] = idx - a * (a + 1) / 2;
    }
    gmm_v4d acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = gmm_v4d{0.0, 0.0, 0.0, 0.0};
    const int b1 = min((c + 1) * G.bpc, G.nblk);
    for (int b = c * G.bpc; b < b1; b++) {
        __syncthreads();
        gmm_stage_diff(G, Ds, b, G.mu + rk * dp, tid);
        if (tid < GMM_BLOCK) rs[tid] = G.resp[rk * G.npad + (size_t)b * GMM_BLOCK + tid];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (wave + 4 * q < ntl) {   // wave-uniform
                for (int s = 0; s < GMM_BLOCK / 4; s++) {
                    const int p = 4 * s + g;
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rs[p] * Ds[p * GMM_LDD + 16 * ti[q] + li], Ds[p * GMM_LDD + 16 * tj[q] + li], acc[q], 0, 0, 0);
                }
            }
        }
    }
    double *S = G.slab + (rk * G.nchunk + c) * dp * dp;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (wave + 4 * q < ntl)
#pragma unroll
            for (int u = 0; u < 4; u++) S[(size_t)(16 * ti[q] + g + 4 * u) * dp + 16 * tj[q] + li] = acc[q][u];
}

__global__ void __launch_bounds__(256) k_gmm_factor(GmmDev G) {
    __shared__ double S[MEDGP_GMM_MAX_D * GMM_LDD];   // lower: the covariance, then L; strictly upper: L^-T
    __shared__ double dv[MEDGP_GMM_MAX_D];            // diag L
    const int k = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    if (gmm_skip(G, r, GMM_PHASE_ITER) || k >= G.k[r]) return;
    const int d = G.d, dp = G.dp;
    const size_t rk = (size_t)r * G.kmax + k;
    const double nk = G.nk[rk];
    double *cov = G.cov + rk * dp * dp, *P = G.P + rk * dp * dp;
    const double *slab = G.slab + rk * G.nchunk * dp * dp;
    for (int idx = tid; idx < d * d; idx += 256) {
        const int i = idx / d, j = idx - i * d;
        if (j > i) continue;
        double s = 0.0;
        for (int c = 0; c < G.nchunk; c++) s += slab[(size_t)c * dp * dp + i * dp + j];
        s /= nk;
        if (i == j) s += G.reg;
        S[i * GMM_LDD + j] = s;
        cov[i * dp + j] = s;
        cov[j * dp + i] = s;
    }
    // right-looking Cholesky, one column per step; the pivot is read by every thread, so the exit is uniform
    bool bad = false;
    for (int j = 0; j < d; j++) {
        __syncthreads();
        const double piv = S[j * GMM_LDD + j];
        if (!(piv > 0.0)) { bad = true; break; }
        const double ljj = sqrt(piv);
        if (tid == 0) dv[j] = ljj;
        for (int i = j + 1 + tid; i < d; i += 256) S[i * GMM_LDD + j] /= ljj;
        __syncthreads();
        const int m = d - j - 1;
        for (int idx = tid; idx < m * m; idx += 256) {
            const int i = j + 1 + idx / m, c = j + 1 + idx % m;
            if (c <= i) S[i * GMM_LDD + c] -= S[i * GMM_LDD + j] * S[c * GMM_LDD + j];
        }
    }
    if (bad) {
        if (tid == 0) G.cfail[rk] = 1;
        return;
    }
    __syncthreads();
    // column j of L^-1 by forward substitution, thread j; it is row j of P = L^-T and goes to the strictly upper part of S
    if (tid < d) {
        const int j = tid;
        const double xj = 1.0 / dv[j];
        for (int i = j + 1; i < d; i++) {
            double s = S[i * GMM_LDD + j] * xj;
            for (int m = j + 1; m < i; m++) s = fma(S[i * GMM_LDD + m], S[j * GMM_LDD + m], s);
            S[j * GMM_LDD + i] = -s / dv[i];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < dp * dp; idx += 256) {
        const int a = idx / dp, b = idx - a * dp;
        double v = 0.0;
        if (a < d && b < d) v = b > a ? S[a * GMM_LDD + b] : (b == a ? 1.0 / dv[a] : 0.0);
        P[idx] = v;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int j = 0; j < d; j++) s += log(dv[j]);
        G.logdet[rk] = s;
    }
}

// one thread per run
__global__ void __launch_bounds__(64) k_gmm_tail(GmmDev G, int phase, int it) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= G.nruns || gmm_skip(G, r, phase)) return;
    double s = 0.0;
    if (phase != GMM_PHASE_INIT) {
        for (int b = 0; b < G.nblk; b++) s += G.blk_lse[(size_t)r * G.nblk + b];
        s /= G.n;
    }
    if (phase == GMM_PHASE_FINAL) { G.score[r] = s; return; }
    bool failed = false;
    for (int k = 0; k < G.k[r]; k++) failed = failed || G.cfail[(size_t)r * G.kmax + k] != 0;
    if (phase == GMM_PHASE_INIT) {
        G.prev[r] = -INFINITY;
        if (failed) G.status[r] = GMM_FAILED;
        return;
    }
    const double change = s - G.prev[r];
    G.prev[r] = s;
    G.lb[r] = s;
    G.niter[r] = it;
    if (failed) G.status[r] = GMM_FAILED;
    else if (fabs(change) < G.tol) G.status[r] = GMM_CONVERGED;
}
