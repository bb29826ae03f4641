// functional_tables_test.cpp -- CPU test of the host tables of medgp_functional_batch (inference_tables.h): the checker of the two-level
// CSR (check_functional_csr), the internal positions (functional_positions) and the tile builder (build_functional_tiles), against
// brute-force restatements.  Stand-alone (own main, no HIP): built with the host compiler and -fsanitize=address,undefined by
// tests/test_functional_tables.py, so an index mistake -- or a read behind a broken offset -- is caught here and not as an out-of-bounds
// access on a GPU.  Every offset array handed to the checker has exactly the length the interface promises.
#include "inference_tables.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {
// two size classes, largest first (ld = 192 with two entries, ld = 64 with three), a scrambled caller order
const std::vector<TableClass> kCls = {{0, 2, 192}, {2, 3, 64}};
const int kOrder[5] = {3, 0, 4, 1, 2};   // internal entry -> caller entry
const int kNb = 5;

unsigned long long rng_state = 88172645463325252ull;
int rnd(int n) {   // xorshift
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (int)(rng_state % (unsigned long long)n);
}

// term count of functional f in pattern `pat`: none, one each, many, or a mix of 0 / 1 / 2 / 25 / 70
int term_count(int pat, int64_t f) {
    const int mixv[5] = {0, 1, 2, 25, 70};
    switch (pat) {
    case 0: return 0;
    case 1: return 1;
    case 2: return 70 + (int)(f % 3);
    default: return mixv[rnd(5)];
    }
}

struct Brute {
    std::vector<PostTile> tiles;
    std::vector<TileChunk> chunks;
    size_t work_need = 0;
    std::vector<int64_t> pos;
};
// brute force: walk the classes, their internal entries and every functional of each, numbering them as they come; a tile closes at 64
// functionals or the patient's end, a chunk when the next tile would pass the budget (a single tile is always let through) or the class ends
Brute brute(const std::vector<int64_t> &foff, size_t budget) {
    Brute R;
    R.pos.assign((size_t)foff[kNb], -1);
    int64_t next = 0;
    for (size_t ci = 0; ci < kCls.size(); ci++) {
        const size_t stride = (size_t)kCls[ci].ld * 64;
        int open = -1;
        auto close = [&]() {
            if (open < 0) return;
            const int nt = (int)R.tiles.size() - open;
            R.chunks.push_back({(int)ci, open, nt, stride, 0, 0, 0, 0, 0, 0});
            R.work_need = std::max(R.work_need, (size_t)nt * stride * sizeof(double));
            open = -1;
        };
        for (int i = kCls[ci].b0; i < kCls[ci].b0 + kCls[ci].count; i++) {
            const int b = kOrder[i];
            PostTile cur{i - kCls[ci].b0, 0, 0, 0};
            for (int64_t f = foff[b]; f < foff[b + 1]; f++) {
                R.pos[(size_t)f] = next++;
                if (cur.cnt == 0) cur.p0 = (int)f;
                cur.cnt++;
                if (cur.cnt == 64 || f + 1 == foff[b + 1]) {
                    if (open >= 0 && ((size_t)((int)R.tiles.size() - open) + 1) * stride * sizeof(double) > budget) close();
                    if (open < 0) open = (int)R.tiles.size();
                    R.tiles.push_back(cur);
                    cur.cnt = 0;
                }
            }
        }
        close();
    }
    return R;
}

FunctionalCsrError run(const std::vector<int64_t> &foff, const std::vector<int64_t> &toff, int64_t *at = nullptr) {
    FunctionalCsr S;
    const FunctionalCsrError e = check_functional_csr(foff.data(), toff.data(), kNb, S);
    if (at) *at = S.at;
    if (e != FUNC_CSR_OK) CHECK(S.F == 0 && S.T == 0 && S.toff.empty() && S.fun.empty());
    return e;
}
}  // namespace

int main() {
    int cases = 0, cut = 0, over = 0;
    // functional counts on and around the tile width, and several tiles
    const int counts[7] = {0, 1, 63, 64, 65, 130, 200};
    const int nc = 7;
    const size_t tile192 = (size_t)192 * 64 * sizeof(double), tile64 = (size_t)64 * 64 * sizeof(double);
    for (int rot = 0; rot < nc; rot++)
        for (int pat = 0; pat < 4; pat++) {
            std::vector<int64_t> foff(kNb + 1, 0);
            for (int b = 0; b < kNb; b++) foff[b + 1] = foff[b] + counts[(b + rot) % nc];
            const int64_t F = foff[kNb];
            std::vector<int64_t> toff((size_t)F + 1, 0);
            for (int64_t f = 0; f < F; f++) toff[(size_t)f + 1] = toff[(size_t)f] + term_count(pat, f);
            // the checker and the staged layout
            FunctionalCsr S;
            CHECK(check_functional_csr(foff.data(), toff.data(), kNb, S) == FUNC_CSR_OK);
            CHECK(S.F == F && S.T == toff[(size_t)F] && S.at == -1 && (int64_t)S.toff.size() == F + 1 && (int64_t)S.fun.size() == S.T);
            for (int64_t f = 0; f <= F; f++) CHECK(S.toff[(size_t)f] == toff[(size_t)f]);
            for (int64_t x = 0; x < S.T; x++) {   // brute force: the one functional whose range holds term x
                int64_t owner = -1;
                for (int64_t f = 0; f < F; f++)
                    if (toff[(size_t)f] <= x && x < toff[(size_t)f + 1]) { CHECK(owner < 0); owner = f; }
                CHECK(owner >= 0 && S.fun[(size_t)x] == owner);
            }
            // positions and tiles
            for (size_t budget : {(size_t)1 << 30, 3 * tile192, 3 * tile64, tile64, (size_t)1}) {
                PointTables<PostTile> T;
                build_functional_tiles(kCls, kOrder, foff.data(), budget, T);
                std::vector<int64_t> pos;
                functional_positions(kCls, kOrder, foff.data(), pos);
                const Brute R = brute(foff, budget);
                CHECK(T.tiles.size() == R.tiles.size() && T.chunks.size() == R.chunks.size() && T.work_need == R.work_need);
                CHECK(pos.size() == R.pos.size());
                std::vector<int> seen((size_t)F, 0);
                for (int64_t f = 0; f < F; f++) {
                    CHECK(pos[(size_t)f] == R.pos[(size_t)f] && pos[(size_t)f] >= 0 && pos[(size_t)f] < F);
                    seen[(size_t)pos[(size_t)f]]++;
                }
                for (int v : seen) CHECK(v == 1);   // a permutation of the functionals
                std::vector<int> cover((size_t)F, 0);
                int64_t walk = 0;
                for (size_t k = 0; k < T.tiles.size(); k++) {
                    const PostTile &a = T.tiles[k], &b = R.tiles[k];
                    CHECK(a.e == b.e && a.p0 == b.p0 && a.cnt == b.cnt && a.pad == 0);
                    CHECK(a.cnt >= 1 && a.cnt <= FUNC_TW && a.p0 >= 0 && (int64_t)a.p0 + a.cnt <= F);
                    // the kernel reads toff[p0 .. p0 + cnt] and the terms between: inside the staged arrays
                    CHECK((size_t)a.p0 + a.cnt < S.toff.size() && S.toff[(size_t)a.p0 + a.cnt] <= S.T && S.toff[a.p0] <= S.toff[(size_t)a.p0 + a.cnt]);
                    for (int c = 0; c < a.cnt; c++) { cover[(size_t)a.p0 + c]++; CHECK(pos[(size_t)a.p0 + c] == walk++); }   // the tiles walk the positions in order
                }
                for (int v : cover) CHECK(v == 1);   // every functional of the call in exactly one column
                for (size_t k = 0; k < T.chunks.size(); k++) {
                    const TileChunk &a = T.chunks[k], &b = R.chunks[k];
                    CHECK(a.cls == b.cls && a.t0 == b.t0 && a.nt == b.nt && a.stride == b.stride && a.stride == (size_t)kCls[a.cls].ld * 64);
                    const size_t bytes = (size_t)a.nt * a.stride * sizeof(double);
                    CHECK(bytes <= budget || a.nt == 1);
                    if (bytes > budget) over++;
                    // the chunks of a class are consecutive and so are their tiles (one k_functional_prep launch per class)
                    if (k > 0 && T.chunks[k - 1].cls == a.cls) CHECK(T.chunks[k - 1].t0 + T.chunks[k - 1].nt == a.t0);
                    if (k > 0) CHECK(T.chunks[k - 1].cls <= a.cls);
                }
                if (T.chunks.size() > kCls.size()) cut++;
                if (budget == (size_t)1) CHECK(T.chunks.size() == T.tiles.size());   // one tile per chunk
                cases++;
            }
        }
    // no functional at all: toffsets is its one value; no tile, no chunk, no work rows
    {
        const std::vector<int64_t> foff(kNb + 1, 0), toff(1, 0);
        CHECK(run(foff, toff) == FUNC_CSR_OK);
        PointTables<PostTile> T;
        build_functional_tiles(kCls, kOrder, foff.data(), tile64, T);
        CHECK(T.tiles.empty() && T.chunks.empty() && T.work_need == 0);
        std::vector<int64_t> pos;
        functional_positions(kCls, kOrder, foff.data(), pos);
        CHECK(pos.empty());
    }
    // broken offsets of every kind; the arrays have exactly the promised length, or -- behind a broken foffsets -- one value
    {
        int64_t at = -2;
        FunctionalCsr S;
        const std::vector<int64_t> good_f = {0, 2, 2, 3, 3, 4}, good_t = {0, 1, 1, 26, 28};
        CHECK(run(good_f, good_t, &at) == FUNC_CSR_OK && at == -1);
        CHECK(check_functional_csr(nullptr, good_t.data(), kNb, S) == FUNC_CSR_NULL);
        CHECK(check_functional_csr(good_f.data(), nullptr, kNb, S) == FUNC_CSR_NULL);
        CHECK(check_functional_csr(nullptr, nullptr, kNb, S) == FUNC_CSR_NULL);
        const std::vector<int64_t> one = {0};
        CHECK(run({1, 2, 2, 3, 3, 4}, one, &at) == FUNC_CSR_FIRST && at == 0);
        CHECK(run({-1, 2, 2, 3, 3, 4}, one, &at) == FUNC_CSR_FIRST && at == 0);
        for (int b = 0; b < kNb; b++) {   // a decrease at every place
            std::vector<int64_t> f = {0, 10, 20, 30, 40, 50};
            f[(size_t)b + 1] = f[b] - 1;
            CHECK(run(f, one, &at) == FUNC_CSR_DECREASE && at == b);
        }
        CHECK(run({0, 0, 0, 0, 0, -1}, one, &at) == FUNC_CSR_DECREASE && at == 4);
        CHECK(run({0, 0, 0, 0, 0, FUNC_MAX_FUNCTIONALS + 1}, one, &at) == FUNC_CSR_COUNT);
        CHECK(run({0, 0, 0, 0, 0, (int64_t)1 << 40}, one, &at) == FUNC_CSR_COUNT);
        CHECK(run(good_f, {1, 1, 1, 26, 28}, &at) == FUNC_CSR_TERM_FIRST && at == 0);
        CHECK(run(good_f, {-3, 1, 1, 26, 28}, &at) == FUNC_CSR_TERM_FIRST && at == 0);
        for (int f = 0; f < 4; f++) {
            std::vector<int64_t> t = {0, 10, 20, 30, 40};
            t[(size_t)f + 1] = t[f] - 1;
            CHECK(run(good_f, t, &at) == FUNC_CSR_TERM_DECREASE && at == f);
        }
        CHECK(run(good_f, {0, 1, 1, FUNC_MAX_TERMS + 1, FUNC_MAX_TERMS + 2}, &at) == FUNC_CSR_TERM_COUNT && at == 2);
        CHECK(run(good_f, {0, 1, 1, 26, (int64_t)1 << 40}, &at) == FUNC_CSR_TERM_COUNT && at == 3);
        // the limits themselves are what the device's ints hold
        CHECK(FUNC_MAX_FUNCTIONALS + FUNC_TW == (int64_t)INT32_MAX && FUNC_MAX_TERMS == (int64_t)INT32_MAX && FUNC_TW == 64);
    }
    CHECK(cut > 0 && over > 0);   // the budgets did cut chunks, and the one-byte budget did leave single tiles above it
    std::printf("functional_tables ok: %d cases, %d with cut chunks\n", cases, cut);
    return 0;
}
