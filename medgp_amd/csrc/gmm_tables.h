// gmm_tables.h -- the launch geometry and buffer sizes of medgp_gmm_fit (kernels_gmm.h).  HOST ONLY: no HIP include, so that
// gmm_tables_test.cpp can check it with the host compiler under sanitizers (make gmm_tables_test; tests/test_gmm_tables.py).
//
// Everything a run's summation order depends on is a function of n and d ALONE (never of the other runs of the call, of kmax or
// of the polling interval): that is what makes a run's bits independent of its call-mates.
#pragma once
#include <cstddef>
#include <cstdint>

#define MEDGP_GMM_MAX_D 80        // features per point (the reference's 73, padded to the 16-wide MFMA tile)
#define MEDGP_GMM_MAX_K 16        // components per run
#define GMM_BLOCK 64              // points per E-step workgroup
#define GMM_MAX_CHUNKS 32         // per-(run, component) partial sums of the M-step: at most this many d x d slabs

struct GmmPlan {
    int dp = 0;         // d rounded up to a multiple of 16
    int nblk = 0;       // 64-point blocks
    int npad = 0;       // nblk * 64: rows of the padded point matrix
    int bpc = 0;        // blocks per M-step chunk
    int nchunk = 0;     // M-step chunks: ceil(nblk / bpc) <= GMM_MAX_CHUNKS
    // element counts of the device buffers (doubles unless said otherwise)
    int64_t x_elems = 0;       // [npad, dp]
    int64_t resp_elems = 0;    // [nruns, kmax, npad]: log-probabilities, then responsibilities
    int64_t par_elems = 0;     // [nruns, kmax, dp]: means
    int64_t mat_elems = 0;     // [nruns, kmax, dp, dp]: covariances; P = L^-T
    int64_t blk_elems = 0;     // [nruns, kmax, nblk]: per-block partial sums of r_ik
    int64_t lse_elems = 0;     // [nruns, nblk]
    int64_t sx_elems = 0;      // [nruns, kmax, nchunk, dp]
    int64_t slab_elems = 0;    // [nruns, kmax, nchunk, dp, dp]
    int64_t label_elems = 0;   // [nruns, n] int32: label0 in, assign out
    int64_t bytes = 0;         // all of it
};

// false: an argument outside the limits
inline bool gmm_plan(int n, int d, int nruns, int kmax, GmmPlan *out) {
    if (n < 2 || d < 1 || d > MEDGP_GMM_MAX_D || nruns < 1 || nruns > 65535 || kmax < 1 || kmax > MEDGP_GMM_MAX_K) return false;
    if (n > INT32_MAX - GMM_BLOCK) return false;
    GmmPlan p;
    p.dp = (d + 15) / 16 * 16;
    p.nblk = (n + GMM_BLOCK - 1) / GMM_BLOCK;
    p.npad = p.nblk * GMM_BLOCK;
    p.bpc = (p.nblk + GMM_MAX_CHUNKS - 1) / GMM_MAX_CHUNKS;
    p.nchunk = (p.nblk + p.bpc - 1) / p.bpc;
    const int64_t rk = (int64_t)nruns * kmax;   // < 2^20, npad < 2^31, nchunk * dp * dp < 2^18: no product below leaves int64
    p.x_elems = (int64_t)p.npad * p.dp;
    p.resp_elems = rk * p.npad;
    p.par_elems = rk * p.dp;
    p.mat_elems = rk * p.dp * p.dp;
    p.blk_elems = rk * p.nblk;
    p.lse_elems = (int64_t)nruns * p.nblk;
    p.sx_elems = rk * p.nchunk * p.dp;
    p.slab_elems = rk * p.nchunk * p.dp * p.dp;
    p.label_elems = (int64_t)nruns * n;
    p.bytes = 8 * (p.x_elems + p.resp_elems + p.par_elems + 2 * p.mat_elems + p.blk_elems + p.lse_elems + p.sx_elems + p.slab_elems) +
              4 * p.label_elems;
    *out = p;
    return true;
}

// the blocks [b0, b1) of M-step chunk c
inline void gmm_chunk_blocks(const GmmPlan &p, int c, int *b0, int *b1) {
    *b0 = c * p.bpc;
    *b1 = (c + 1) * p.bpc < p.nblk ? (c + 1) * p.bpc : p.nblk;
}

// the lower-triangle 16 x 16 tile (ti >= tj) number idx of a dp x dp matrix, row by row: (0,0) (1,0) (1,1) (2,0) ...
inline void gmm_lower_tile(int idx, int *ti, int *tj) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= idx) i++;
    *ti = i;
    *tj = idx - i * (i + 1) / 2;
}
