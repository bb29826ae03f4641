// fisher_tables_test.cpp -- CPU test of fisher_tables.h: the workgroup -> tile maps of k_fisher_t (all tiles) and k_fisher_kdot (lower
// tiles), the element ranges those kernels and k_fisher_wgrad address inside a class's matrix buffers, the buffer sizes and the
// capacity rule, against brute-force restatements.  Stand-alone (own main, no HIP): built with the host compiler and
// -fsanitize=address,undefined by tests/test_fisher.py, so an index mistake shows here and not as an out-of-bounds access on a GPU.
// The buffers are real allocations of the computed sizes, written at every address the kernels write: the sanitizer checks the bounds.
// Build and run: make fisher_tables_test && ./fisher_tables_test
#include "call_plan.h"
#include "fisher_tables.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

// one call: lay out the plan, size the buffers, walk every workgroup of the two tile launches of every class and touch what it stores
int run_call(const std::vector<int> &en, int Q, int D, int H, int nvec, size_t budget) {
    PlanRules r;
    r.Q = Q; r.D = D; r.max_batch = (int)en.size(); r.mem_budget = budget;
    BatchPlan P;
    layout_plan(r, en.data(), (int)en.size(), true, P);
    if (P.nwaves > 1 || !fisher_fits(P.need_mat, budget)) return 0;
    CHECK((size_t)FISHER_MATS * P.need_mat * sizeof(double) <= budget);
    const FisherBuffers fb = fisher_buffers(P.need_mat, (int)en.size(), nvec, H, Q, D);
    CHECK(fb.mat_doubles == P.need_mat);
    CHECK(fb.coef_doubles == en.size() * ((size_t)D + (size_t)Q * D * D + 2 * (size_t)Q));
    CHECK(fb.dir_doubles == en.size() * (size_t)nvec * (size_t)H);
    std::vector<char> kdot(fb.mat_doubles, 0), tm(fb.mat_doubles, 0);   // one byte per double: 0 untouched, 1 stored once
    size_t covered = 0;
    for (const SizeClass &k : P.cls) {
        CHECK(k.off_mat + (size_t)k.count * k.ld * k.ld <= fb.mat_doubles);
        const int nt64 = k.nbmax;
        CHECK(64 * nt64 == k.ld);
        for (int b = 0; b < k.count; b++) {
            const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64, nb = npad / 64;
            CHECK(npad <= k.ld);
            const size_t base = k.off_mat + (size_t)b * k.ld * k.ld;
            // k_fisher_kdot: lower tiles, each storing itself and its mirror image
            std::vector<int> seen((size_t)nt64 * nt64, 0);
            for (int x = 0; x < fisher_kdot_grid(nt64); x++) {
                int I, J;
                fisher_lower_tile(x, I, J);
                CHECK(I >= 0 && I < nt64 && J >= 0 && J <= I);
                seen[(size_t)I * nt64 + J]++;
                if (I >= nb) continue;
                for (int rr = 0; rr < 64; rr++)
                    for (int cc = 0; cc < 64; cc++) {
                        kdot[base + (size_t)(64 * I + rr) * k.ld + 64 * J + cc]++;
                        if (I != J) kdot[base + (size_t)(64 * J + rr) * k.ld + 64 * I + cc]++;
                    }
            }
            for (int I = 0; I < nt64; I++)
                for (int J = 0; J < nt64; J++) CHECK(seen[(size_t)I * nt64 + J] == (J <= I ? 1 : 0));
            // k_fisher_t: all tiles
            std::fill(seen.begin(), seen.end(), 0);
            for (int x = 0; x < fisher_t_grid(nt64); x++) {
                int I, J;
                fisher_t_tile(x, nt64, I, J);
                CHECK(I >= 0 && I < nt64 && J >= 0 && J < nt64);
                seen[(size_t)I * nt64 + J]++;
                if (64 * I >= npad || 64 * J >= npad) continue;
                for (int rr = 0; rr < 64; rr++)
                    for (int cc = 0; cc < 64; cc++) tm[base + (size_t)(64 * I + rr) * k.ld + 64 * J + cc]++;
            }
            for (int v : seen) CHECK(v == 1);
            // every element of [0, npad)^2 stored exactly once, nothing outside it: what k_fisher_t and k_fisher_wgrad then read
            // (rows 64 I .., columns [0, npad)) is written
            for (int i = 0; i < k.ld; i++)
                for (int j = 0; j < k.ld; j++) {
                    const int want = (i < npad && j < npad) ? 1 : 0;
                    CHECK(kdot[base + (size_t)i * k.ld + j] == want && tm[base + (size_t)i * k.ld + j] == want);
                }
            covered += (size_t)npad * npad;
        }
    }
    CHECK(covered > 0);
    return 1;
}
}  // namespace

int main() {
    int ran = 0, refused = 0;
    const std::vector<std::vector<int>> calls = {
        {1}, {3, 63, 64, 65}, {130, 200, 1, 64, 65, 512}, {200, 130}, {320, 257, 64, 64, 700}};
    for (const auto &en : calls)
        for (size_t budget : {(size_t)64 << 10, (size_t)1 << 20, (size_t)3 << 20, (size_t)64 << 20}) {
            const int r = run_call(en, 2, 3, 25, 2, budget);
            ran += r; refused += !r;
        }
    CHECK(ran >= 6 && refused >= 6);
    // the rule at its edge: exactly FISHER_MATS matrices of 8-byte doubles
    CHECK(fisher_fits(4096, (size_t)FISHER_MATS * 4096 * 8) && !fisher_fits(4097, (size_t)FISHER_MATS * 4096 * 8) && fisher_fits(0, 0));
    std::printf("fisher_tables ok (%d calls walked, %d refused)\n", ran, refused);
    return 0;
}
