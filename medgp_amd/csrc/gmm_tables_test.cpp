// CPU test of gmm_tables.h (the launch geometry and buffer sizes of medgp_gmm_fit): plain C++, host compiler, sanitizers; no GPU.
// Build and run: make gmm_tables_test && ./gmm_tables_test   (tests/test_gmm_tables.py does both)
#include "gmm_tables.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static void check_plan(int n, int d, int nruns, int kmax) {
    GmmPlan p;
    CHECK(gmm_plan(n, d, nruns, kmax, &p));
    CHECK(p.dp % 16 == 0 && p.dp >= d && p.dp - d < 16 && p.dp <= MEDGP_GMM_MAX_D);
    CHECK(p.npad % GMM_BLOCK == 0 && p.npad >= n && p.npad - n < GMM_BLOCK && p.nblk * GMM_BLOCK == p.npad);
    CHECK(p.nchunk >= 1 && p.nchunk <= GMM_MAX_CHUNKS && p.bpc >= 1);
    // the chunks cover every block exactly once, in order, and none is empty: mark the blocks a real buffer of nblk entries
    std::vector<int> seen((size_t)p.nblk, 0);
    int next = 0;
    for (int c = 0; c < p.nchunk; c++) {
        int b0, b1;
        gmm_chunk_blocks(p, c, &b0, &b1);
        CHECK(b0 == next && b1 > b0 && b1 <= p.nblk);
        for (int b = b0; b < b1; b++) seen[(size_t)b]++;
        next = b1;
    }
    CHECK(next == p.nblk);
    for (int b = 0; b < p.nblk; b++) CHECK(seen[(size_t)b] == 1);
    // the geometry depends on n and d alone
    GmmPlan q;
    CHECK(gmm_plan(n, d, 1, 1, &q));
    CHECK(q.dp == p.dp && q.nblk == p.nblk && q.npad == p.npad && q.bpc == p.bpc && q.nchunk == p.nchunk);
    // sizes: the largest index each kernel forms, restated, is the last element
    const int64_t rk = (int64_t)nruns * kmax;
    CHECK(p.x_elems == ((int64_t)(p.npad - 1) * p.dp + p.dp - 1) + 1);
    CHECK(p.resp_elems == ((rk - 1) * p.npad + p.npad - 1) + 1);
    CHECK(p.par_elems == ((rk - 1) * p.dp + p.dp - 1) + 1);
    CHECK(p.mat_elems == ((rk - 1) * p.dp * p.dp + (int64_t)(p.dp - 1) * p.dp + p.dp - 1) + 1);
    CHECK(p.blk_elems == ((rk - 1) * p.nblk + p.nblk - 1) + 1);
    CHECK(p.lse_elems == ((int64_t)(nruns - 1) * p.nblk + p.nblk - 1) + 1);
    CHECK(p.sx_elems == (((rk - 1) * p.nchunk + p.nchunk - 1) * p.dp + p.dp - 1) + 1);
    CHECK(p.slab_elems == (((rk - 1) * p.nchunk + p.nchunk - 1) * p.dp * p.dp + (int64_t)p.dp * p.dp - 1) + 1);
    CHECK(p.label_elems == ((int64_t)(nruns - 1) * n + n - 1) + 1);
    CHECK(p.bytes > 0 && p.bytes >= 8 * (p.resp_elems + p.slab_elems));
}

int main() {
    const int ns[] = {2, 5, 63, 64, 65, 130, 300, 2047, 2048, 2049, 20480, 64 * 32, 64 * 32 + 1, 64 * 33, 1000003, INT32_MAX - GMM_BLOCK};
    const int ds[] = {1, 2, 15, 16, 17, 32, 73, MEDGP_GMM_MAX_D};
    for (int n : ns)
        for (int d : ds) {
            check_plan(n, d, 1, 1);
            check_plan(n, d, 12, 5);
            check_plan(n, d, 50, MEDGP_GMM_MAX_K);
        }
    check_plan(INT32_MAX - GMM_BLOCK, MEDGP_GMM_MAX_D, 65535, MEDGP_GMM_MAX_K);   // the largest call: nothing wraps
    GmmPlan p;
    CHECK(!gmm_plan(1, 2, 1, 1, &p) && !gmm_plan(10, 0, 1, 1, &p) && !gmm_plan(10, MEDGP_GMM_MAX_D + 1, 1, 1, &p));
    CHECK(!gmm_plan(10, 2, 0, 1, &p) && !gmm_plan(10, 2, 65536, 1, &p) && !gmm_plan(10, 2, 1, 0, &p) && !gmm_plan(10, 2, 1, MEDGP_GMM_MAX_K + 1, &p));
    CHECK(!gmm_plan(INT32_MAX, 2, 1, 1, &p));
    // the pricing shape: 20480 x 73, 50 runs of up to 5 components stays far inside the default 8 GB
    CHECK(gmm_plan(20480, 73, 50, 5, &p) && p.nblk == 320 && p.bpc == 10 && p.nchunk == 32 && p.bytes < ((int64_t)1 << 30));
    // lower tiles: row by row, each exactly once
    for (int nt = 1; nt <= MEDGP_GMM_MAX_D / 16; nt++) {
        int idx = 0;
        for (int i = 0; i < nt; i++)
            for (int j = 0; j <= i; j++, idx++) {
                int ti, tj;
                gmm_lower_tile(idx, &ti, &tj);
                CHECK(ti == i && tj == j);
            }
        CHECK(idx == nt * (nt + 1) / 2 && idx <= 16);   // k_gmm_cov gives each of its 4 waves at most 4 tiles
    }
    std::printf("gmm_tables ok\n");
    return 0;
}
