// warp_tables_test.cpp -- CPU test of warp_tables.h (plain C++, host compiler, sanitizers; no GPU, no HIP): the buffers of a warp call
// hold regions that do not overlap, every index the kernels form through the element maps stays inside its region, and the cut of
// k_warp_solve reads every element of the upper triangle of U exactly once per product, inside the entry's matrix, in 16-byte pairs.
#include "warp_tables.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);          \
            if (++fails > 20) std::exit(1);                                   \
        }                                                                     \
    } while (0)

static int roundup(int x, int m) { return (x + m - 1) / m * m; }

// marks [off, off + len) of a buffer of `size` elements; an element marked twice or outside is an overlap / overrun
static void mark(std::vector<unsigned char> &buf, size_t off, size_t len) {
    CHECK(off + len <= buf.size());
    for (size_t i = off; i < off + len && i < buf.size(); i++) {
        CHECK(buf[i] == 0);
        buf[i] = 1;
    }
}

// the two products of k_warp_solve on an entry of n rows in a view of leading dimension ld: counts the reads of every element of U
static void walk_solve(int n, int ld) {
    const int npad = roundup(n, 64);
    CHECK(npad <= ld);
    std::vector<int> seen((size_t)ld * ld, 0);
    const int ncb = warp_solve_blocks(npad);
    std::vector<int> wrote(ld, 0);
    for (int cb = 0; cb < ncb; cb++) {
        for (int c = 0; c < WARP_SOLVE_CLASSES; c++)
            for (int lane = 0; lane < 64; lane++) {
                const int i0 = warp_solve_col(cb, lane), j1 = warp_solve_rows(cb, n);
                CHECK(i0 % 2 == 0);
                if (i0 >= npad) continue;
                CHECK(i0 + 1 < ld);
                for (int j = c; j < j1; j += WARP_SOLVE_CLASSES) {
                    if (j > i0 + 1) continue;
                    CHECK(j >= 0 && j < n);
                    const size_t at = (size_t)j * ld + i0;
                    CHECK(at + 1 < seen.size() && at % 2 == 0);   // one aligned 16-byte load
                    if (j <= i0) seen[at]++;
                    seen[at + 1]++;
                }
            }
        for (int tid = 0; tid < WARP_SOLVE_COLS; tid++) {
            const int i = cb * WARP_SOLVE_COLS + tid;
            if (i < npad) { CHECK(i < ld); wrote[i]++; }
        }
    }
    for (int i = 0; i < npad; i++) CHECK(wrote[i] == 1);
    // every (row <= column < n) once -- columns n .. npad are read and masked to zero by the kernel (w is zero there)
    for (int j = 0; j < n; j++)
        for (int i = j; i < n; i++) CHECK(seen[(size_t)j * ld + i] == 1);
    for (int j = 0; j < ld; j++)
        for (int i = 0; i < j && i < ld; i++) CHECK(seen[(size_t)j * ld + i] == 0);   // nothing below the diagonal is used
    // the second product
    std::vector<int> seen2((size_t)ld * ld, 0);
    for (int j = 0; j < npad; j++) {
        if (j >= n) continue;
        for (int cb = warp_solve_first_block(j); cb < ncb; cb++)
            for (int lane = 0; lane < 64; lane++) {
                const int i0 = warp_solve_col(cb, lane);
                if (!(i0 < npad && i0 + 1 >= j && i0 < n)) continue;
                CHECK(i0 + 1 < ld);
                const size_t at = (size_t)j * ld + i0;
                CHECK(at + 1 < seen2.size() && at % 2 == 0);
                if (i0 >= j) seen2[at]++;
                if (i0 + 1 < n) seen2[at + 1]++;
            }
    }
    for (int j = 0; j < n; j++)
        for (int i = 0; i < ld; i++) CHECK(seen2[(size_t)j * ld + i] == ((i >= j && i < n) ? 1 : 0));
}

int main() {
    const int Ds[] = {1, 3, 24, 64}, nqs[] = {0, 1, 64};
    for (int n = 1; n <= 300; n++) {
        // a class of three entries whose largest is n (the view's ld: n rounded up to 64), and one wider view
        for (int ld : {roundup(n, 64), roundup(n, 64) + 64}) {
            walk_solve(n, ld);
            if (n > 1) walk_solve(n - 1, ld);
        }
        const int ld = roundup(n, 64), nbatch = 3;
        const size_t need_vec = (size_t)nbatch * ld + 128;   // (a second class behind this one)
        for (int D : Ds)
            for (int nq : nqs) {
                const size_t M = (size_t)(n % 7) * 5;        // 0 points included
                const WarpBuffers wb = warp_buffers(need_vec, nbatch, D, M, nq);
                // the vector buffer: four roles, entries ld apart, rows below ld
                std::vector<unsigned char> vec(wb.vec_doubles, 0);
                for (int r = 0; r < WARP_VECS; r++)
                    for (int e = 0; e < nbatch; e++) mark(vec, warp_vec_offset(r, need_vec) + warp_vec_at(e, ld, 0), (size_t)ld);
                CHECK(warp_vec_at(nbatch - 1, ld, ld - 1) < need_vec);
                // the small blocks
                std::vector<unsigned char> sm(wb.small_doubles, 0);
                for (int e = 0; e < nbatch; e++) {
                    const size_t base = (size_t)e * warp_small_stride(D);
                    mark(sm, base + warp_off_logjac(), 1);
                    mark(sm, base + warp_off_quad(), 1);
                    for (int d = 0; d < D; d++)
                        for (int k = 0; k < WARP_NPSI; k++) mark(sm, base + warp_off_dpsi(d, k), 1);
                }
                for (size_t i = 0; i < sm.size(); i++) CHECK(sm[i] == 1);
                // the inputs
                std::vector<unsigned char> in(wb.in_doubles, 0);
                for (int pos = 0; pos < nbatch; pos++)
                    for (int d = 0; d < D; d++)
                        for (int k = 0; k < WARP_NPSI; k++) mark(in, warp_in_psi(pos, D, d, k), 1);
                mark(in, warp_in_zq(nbatch, D), (size_t)nq);
                CHECK(nq <= WARP_MAX_NQ);
                // the per-point outputs
                const size_t Mz = M > 0 ? M : 1;
                std::vector<unsigned char> out(wb.out_doubles, 0);
                mark(out, warp_out_zmean(Mz), Mz);
                mark(out, warp_out_zvar(Mz), Mz);
                mark(out, warp_out_lpd(Mz), Mz);
                for (size_t pt = 0; pt < M; pt++)
                    for (int k = 0; k < nq; k++) mark(out, warp_out_quant(Mz) + warp_quant_at(pt, nq, k), 1);
            }
    }
    // the capacity rule: what it admits fits, one double more of vectors does not
    {
        const size_t budget = (size_t)1 << 20, lim = budget / sizeof(double);
        const size_t mat = 40000, vecmax = (lim - WARP_MATS * mat) / WARP_VECS;
        CHECK(warp_fits(mat, vecmax, budget));
        CHECK(!warp_fits(mat, vecmax + 1, budget));
        CHECK(!warp_fits(lim / WARP_MATS + 1, 0, budget));
        CHECK(WARP_MATS * mat + WARP_VECS * vecmax <= lim);
    }
    if (fails) {
        std::printf("warp_tables_test: %d failures\n", fails);
        return 1;
    }
    std::printf("warp_tables_test: ok\n");
    return 0;
}
