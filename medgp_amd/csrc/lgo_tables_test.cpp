// lgo_tables_test.cpp -- CPU test of build_lgo_tables (inference_tables.h): the per-workgroup rows and per-entry tables that
// medgp_lgo_grad's own kernels read, against brute-force restatements.  Stand-alone (own main, no HIP): built with the host compiler and
// -fsanitize=address,undefined by tests/test_lgo_grad.py, so an index mistake in the builder is caught here and not as an out-of-bounds
// access on a GPU.  It also walks the index ranges the kernels form from a row (k_lgo_inv, k_lgo_s, k_lgo_t) inside the group's block.
// Build and run: make lgo_tables_test && ./lgo_tables_test
#include "inference_tables.h"

#include <cstdio>
#include <cstdlib>
#include <random>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {
// two size classes, largest first (ld = 256 with two entries, ld = 64 with three), a scrambled caller order
const std::vector<TableClass> kCls = {{0, 2, 256}, {2, 3, 64}};
const int kOrder[5] = {3, 0, 4, 1, 2};   // internal entry -> caller entry
const int kNb = 5;
const int kEn[5] = {200, 130, 64, 40, 1};

int run_case(std::mt19937 &rng, int scheme, size_t budget) {
    std::vector<int64_t> ooff(kNb + 1, 0), goff(kNb + 1, 0);
    std::vector<int> nobs(kNb), ng(kNb);
    for (int i = 0; i < kNb; i++) nobs[kOrder[i]] = kEn[i];
    for (int b = 0; b < kNb; b++) {
        ng[b] = scheme == 0 ? nobs[b] : (scheme == 1 ? 1 : (scheme == 2 ? 0 : 6));
        ooff[b + 1] = ooff[b] + nobs[b];
        goff[b + 1] = goff[b] + ng[b];
    }
    std::vector<int32_t> group((size_t)ooff[kNb]);
    for (int b = 0; b < kNb; b++)
        for (int o = 0; o < nobs[b]; o++) {
            int g;
            if (scheme == 0) g = o;                                 // all singletons
            else if (scheme == 1) g = 0;                            // one group of everything
            else if (scheme == 2) g = -1;                           // nothing held out
            else if (scheme == 3) g = (int)(rng() % 7) - 1, g = g == 4 ? 3 : g;   // random ids in [-1, 6), id 4 empty
            else g = nobs[b] == 200 ? (o % 3 == 0 ? -1 : (o % 3 == 1 ? 0 : (o < 150 ? 1 : (o == 152 ? 5 : 2)))) : o % 6;   // interleaved large groups, a singleton
            group[(size_t)(ooff[b] + o)] = g;
        }
    std::vector<std::vector<int>> perms(kNb);
    std::vector<const int *> perm(kNb, nullptr);
    for (int b : {kOrder[0], kOrder[3]}) {
        perms[b].resize(nobs[b]);
        for (int r = 0; r < nobs[b]; r++) perms[b][r] = (int)(((long long)r * 7 + 3) % nobs[b]);   // (7 is coprime to 200 and 40)
        perm[b] = perms[b].data();
    }
    LooTables T;
    LgoTables G;
    TableError e{-1, -1, -1, 0, 0};
    if (!build_loo_tables(kCls, kOrder, kEn, ooff.data(), goff.data(), kNb, group.data(), perm.data(), false, true, budget, T, e)) return 0;
    build_lgo_tables(kCls, kEn, T, G);

    // sgl: exactly the singleton rows, with their group of the call; -1 on members of larger groups, id -1 and the padding
    size_t total = 0;
    CHECK(G.sgl_off.size() == kCls.size());
    for (size_t ci = 0; ci < kCls.size(); ci++) { CHECK(G.sgl_off[ci] == total); total += (size_t)kCls[ci].count * kCls[ci].ld; }
    CHECK(G.sgl.size() == total && G.ent.size() == 2 * (size_t)kNb);
    std::vector<int> first((size_t)goff[kNb], -1);   // first internal row of every group of the call
    for (size_t ci = 0; ci < kCls.size(); ci++)
        for (int ee = 0; ee < kCls[ci].count; ee++) {
            const int i = kCls[ci].b0 + ee, b = kOrder[i];
            for (int r = 0; r < kCls[ci].ld; r++) {
                int want = -1;
                if (r < kEn[i]) {
                    const int g = group[(size_t)(ooff[b] + (perm[b] ? perm[b][r] : r))];
                    if (g >= 0) {
                        if (first[(size_t)(goff[b] + g)] < 0) first[(size_t)(goff[b] + g)] = r;
                        if (T.gsize[(size_t)(goff[b] + g)] == 1) want = (int)(goff[b] + g);
                    }
                }
                CHECK(G.sgl[G.sgl_off[ci] + (size_t)ee * kCls[ci].ld + r] == want);
            }
        }
    // ent / gord: per internal entry its non-empty groups, each once, by first member row
    std::vector<int> seen((size_t)goff[kNb], 0);
    int xnext = 0;
    for (int i = 0; i < kNb; i++) {
        const int b = kOrder[i], x0 = G.ent[2 * (size_t)i], x1 = G.ent[2 * (size_t)i + 1];
        CHECK(x0 == xnext && x1 >= x0 && x1 <= (int)G.gord.size());
        xnext = x1;
        int nonempty = 0;
        for (int64_t g = goff[b]; g < goff[b + 1]; g++) nonempty += T.gsize[(size_t)g] > 0;
        CHECK(x1 - x0 == nonempty);
        for (int x = x0; x < x1; x++) {
            const int g = G.gord[(size_t)x];
            CHECK(g >= goff[b] && g < goff[b + 1] && T.gsize[(size_t)g] > 0 && seen[(size_t)g]++ == 0);
            if (x > x0) CHECK(first[(size_t)G.gord[(size_t)x - 1]] < first[(size_t)g]);
        }
    }
    CHECK(xnext == (int)G.gord.size());
    // chunks: rows of cols / trows partition in chunk order; per group nt column tiles and the entry's row blocks, each once; the
    // index ranges of the kernels stay inside the group's block and the entry's matrix
    CHECK(G.chunks.size() == T.chunks.size());
    int cnext = 0, tnext = 0;
    for (size_t x = 0; x < T.chunks.size(); x++) {
        const LooChunk &ch = T.chunks[x];
        const LgoChunk &gc = G.chunks[x];
        const TableClass &k = kCls[(size_t)ch.cls];
        CHECK(gc.col0 == cnext && gc.trow0 == tnext && gc.ncol >= ch.ng && gc.ntrow >= ch.ng);
        cnext += gc.ncol; tnext += gc.ntrow;
        for (int gi = ch.g0; gi < ch.g0 + ch.ng; gi++) {
            const JointPat &P = T.groups[(size_t)gi];
            const int nt = (P.m + 63) / 64, mpad = 64 * nt, n = kEn[k.b0 + P.e], nrb = (n + 63) / 64;
            std::vector<int> cseen((size_t)nt, 0), rseen((size_t)nrb, 0);
            for (int q = gc.col0; q < gc.col0 + gc.ncol; q++)
                if (G.cols[(size_t)q].pat == gi) { CHECK(G.cols[(size_t)q].I >= 0 && G.cols[(size_t)q].I < nt && G.cols[(size_t)q].J == 0); cseen[(size_t)G.cols[(size_t)q].I]++; }
            for (int q = gc.trow0; q < gc.trow0 + gc.ntrow; q++)
                if (G.trows[(size_t)q].pat == gi) { CHECK(G.trows[(size_t)q].I >= 0 && G.trows[(size_t)q].I < nrb); rseen[(size_t)G.trows[(size_t)q].I]++; }
            for (int v : cseen) CHECK(v == 1);
            for (int v : rseen) CHECK(v == 1);
            // the block [R -> S | X | w | -] and what the kernels address in it
            const size_t blk = loo_block_doubles(P.m);
            CHECK((size_t)P.coff * 8 + blk * 8 <= T.blk_need);
            const size_t last_x = (size_t)mpad * mpad + (size_t)(mpad - 1) * mpad + (mpad - 1), last_w = 2 * (size_t)mpad * mpad + (mpad - 1);
            CHECK(last_x < blk && last_w < blk);
            // k_lgo_t: rows 64 rb + 63 < npad <= ld, gathered rows < n
            CHECK(64 * nrb <= k.ld);
            for (int p = 0; p < P.m; p++) CHECK(T.rows[(size_t)(P.p0 + p)].r >= 0 && T.rows[(size_t)(P.p0 + p)].r < n);
        }
    }
    CHECK(cnext == (int)G.cols.size() && tnext == (int)G.trows.size());
    return 1 + (T.chunks.size() > 2 ? 1 : 0);
}
}  // namespace

int main() {
    std::mt19937 rng(20261209);
    int built = 0, cut = 0, refused = 0;
    for (int scheme = 0; scheme < 5; scheme++)
        for (size_t budget : {(size_t)100000, (size_t)300000, (size_t)700000, (size_t)8 << 20}) {
            const int r = run_case(rng, scheme, budget);
            built += r > 0; cut += r > 1; refused += r == 0;
        }
    CHECK(built >= 12 && cut >= 2 && refused >= 2);
    std::printf("lgo_tables ok (%d built, %d with cut chunks, %d refused)\n", built, cut, refused);
    return 0;
}
