// CPU test of forecast_grad_tables.h (the prefix validation and the per-entry integer table of medgp_forecast_grad): plain C++, host
// compiler, sanitizers; no GPU.  The tables are filled into exactly sized heap blocks, so a write past FC_TAB_INTS * ld is caught.
// Build and run: make forecast_grad_tables_test && ./forecast_grad_tables_test   (tests/test_forecast_grad_tables.py does both)
#include "forecast_grad_tables.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// one entry against a brute-force restatement; walks the index ranges the kernels form from the table
static void check_entry(int n, int ld, const std::vector<int32_t> *prefix, const std::vector<int> *perm) {
    std::vector<int> tab((size_t)FC_TAB_INTS * ld, 12345);
    fc_fill_entry(n, ld, prefix ? prefix->data() : nullptr, perm ? perm->data() : nullptr, tab.data());
    const int nblk = ld / 64, npad = (n + 63) / 64 * 64;
    const int *pfx = tab.data(), *gpos = pfx + ld, *pmin = gpos + ld, *pmax = pmin + nblk;
    const int c0 = pmax[nblk], c1 = pmax[nblk + 1], pall = pmax[nblk + 2], nscored = pmax[nblk + 3];
    int count = 0, big = 0, first = -1, last = -1;
    for (int i = 0; i < ld; i++) {
        const int want = i < n ? (prefix ? (*prefix)[i] : i) : FC_NONE;
        CHECK(pfx[i] == (want < 0 ? FC_NONE : want));
        if (want >= 0) { count++; big = std::max(big, want); if (first < 0) first = i / 64; last = i / 64; }
    }
    CHECK(nscored == count && pall == big && pall <= std::max(n - 1, 0));
    CHECK(c0 == (count ? first : 0) && c1 == (count ? last + 1 : 0) && 64 * c1 <= npad);
    for (int C = 0; C < nblk; C++) {
        int lo = FC_EMPTY_MIN, hi = -1;
        for (int i = 64 * C; i < 64 * C + 64; i++)
            if (pfx[i] >= 0) { lo = std::min(lo, pfx[i]); hi = std::max(hi, pfx[i]); }
        CHECK(pmin[C] == lo && pmax[C] == hi);
        if (lo != FC_EMPTY_MIN) {
            CHECK(C >= c0 && C < c1);
            // k_fc_t, tile (R, C), R <= C: the chunked column range starts inside the tile's rows and covers every band of the block
            for (int R = 0; R <= C; R++) {
                const int k0 = std::max(64 * R, lo & ~31), k1 = 64 * C + 64;
                CHECK(k0 >= 0 && k0 < k1 && (k1 - k0) % 32 == 0 && k1 <= npad);
                for (int i = 64 * C; i < 64 * C + 64; i++)
                    if (pfx[i] >= 0) CHECK(std::max(pfx[i], 64 * R) >= k0 && i < k1);
            }
        }
    }
    // gpos: a permutation of [0, n) that inverts perm, the identity behind it
    std::vector<int> seen((size_t)ld, 0);
    for (int j = 0; j < ld; j++) {
        CHECK(gpos[j] >= 0 && gpos[j] < ld);
        seen[(size_t)gpos[j]]++;
        if (j >= n) CHECK(gpos[j] == j);
        else CHECK(gpos[j] < n);
    }
    for (int j = 0; j < ld; j++) CHECK(seen[(size_t)j] == 1);
    for (int g = 0; g < n; g++) CHECK(gpos[perm ? (*perm)[g] : g] == g);
    // k_fc_qm reads S[j, p_i - 1] for j < p_i: inside the scanned range [j, pall) of row j
    for (int i = 0; i < n; i++)
        if (pfx[i] > 0) CHECK(pfx[i] - 1 < pall && pfx[i] - 1 < n);
}

int main() {
    std::mt19937 rng(20261201);
    const int ns[] = {0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 200, 512, 777};
    for (int n : ns) {
        const int npad = std::max(64, (n + 63) / 64 * 64);
        for (int ld : {npad, npad + 64, npad + 192}) {
            check_entry(n, ld, nullptr, nullptr);
            std::vector<int> perm((size_t)n);
            std::iota(perm.begin(), perm.end(), 0);
            std::shuffle(perm.begin(), perm.end(), rng);
            check_entry(n, ld, nullptr, &perm);
            std::vector<int32_t> none((size_t)n, -1), zero((size_t)n, 0), lastonly((size_t)n, -1);
            if (n) lastonly[(size_t)n - 1] = n - 1;
            check_entry(n, ld, &none, &perm);
            check_entry(n, ld, &zero, nullptr);
            check_entry(n, ld, &lastonly, &perm);
            for (int rep = 0; rep < 4; rep++) {
                std::vector<int32_t> p((size_t)n);
                for (int i = 0; i < n; i++) {
                    const int r = (int)(rng() % 4);
                    p[(size_t)i] = r == 0 ? -1 : (r == 1 ? i : (int)(rng() % (unsigned)(i + 1)));
                }
                check_entry(n, ld, &p, rep & 1 ? &perm : nullptr);
            }
        }
    }
    // validation
    const int n2[2] = {3, 2};
    const int64_t off[3] = {0, 3, 5};
    int32_t p[5] = {0, -1, 2, 0, 1};
    FcError e;
    CHECK(fc_check(2, n2, off, p, &e));
    CHECK(fc_check(2, n2, nullptr, nullptr, &e));
    CHECK(fc_check(2, n2, off, nullptr, &e));
    CHECK(!fc_check(2, n2, nullptr, p, &e) && e.b == -1);
    p[1] = 2;   // above i
    CHECK(!fc_check(2, n2, off, p, &e) && e.b == 0 && e.i == 1 && e.value == 2 && e.expect == 1);
    p[1] = -2;
    CHECK(!fc_check(2, n2, off, p, &e) && e.b == 0 && e.i == 1 && e.value == -2);
    p[1] = -1;
    p[3] = 1;   // patient 1, observation 0
    CHECK(!fc_check(2, n2, off, p, &e) && e.b == 1 && e.i == 3 && e.expect == 0);
    p[3] = 0;
    const int64_t shortoff[3] = {0, 2, 5}, badstart[3] = {1, 4, 6}, back[3] = {0, 3, 2};
    CHECK(!fc_check(2, n2, shortoff, p, &e) && e.b == 0 && e.i == -1 && e.value == 2 && e.expect == 3);
    CHECK(!fc_check(2, n2, badstart, p, &e) && e.i == -1);
    CHECK(!fc_check(2, n2, back, p, &e) && e.b == 1 && e.i == -1 && e.value == -1);
    CHECK(!fc_check(2, n2, shortoff, nullptr, &e));
    std::printf("forecast_grad_tables ok\n");
    return 0;
}
