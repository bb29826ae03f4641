// components_tables_test.cpp -- CPU test of build_components_tiles (inference_tables.h) against a brute-force restatement.
// Stand-alone (own main, no HIP): built with the host compiler and -fsanitize=address,undefined by tests/test_components_tables.py, so
// an index mistake in the builder is caught here and not as an out-of-bounds access on a GPU.
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
const int kQs[6] = {1, 2, 3, 5, 17, 64};

// the pairs of a tile, counted one by one: every point of a full tile, every q > r
size_t brute_extra(int Q) {
    size_t np = 0;
    int P = 0;
    while ((P + 1) * Q <= 64) P++;   // the points whose Q columns fit 64 columns
    for (int pt = 0; pt < P; pt++)
        for (int q = 0; q < Q; q++)
            for (int r = 0; r < q; r++) np++;
    return np;
}

// brute force: walk the classes, their internal entries and every point of each; a tile closes when one more point's Q columns would
// not fit its 64 columns or the patient ends, a chunk when the next tile would pass the budget (a single tile is always let through)
// or the class ends
struct Brute {
    std::vector<PostTile> tiles;
    std::vector<TileChunk> chunks;
    size_t work_need = 0;
};
Brute brute(const std::vector<int64_t> &off, int Q, bool with_cov, size_t budget) {
    Brute R;
    for (size_t ci = 0; ci < kCls.size(); ci++) {
        const size_t stride = (size_t)kCls[ci].ld * 64 + (with_cov ? brute_extra(Q) : 0);
        int open = -1;   // first tile of the open chunk
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
            for (int64_t p = off[b]; p < off[b + 1]; p++) {
                if (cur.cnt == 0) cur.p0 = (int)p;
                cur.cnt++;
                if ((cur.cnt + 1) * Q > 64 || p + 1 == off[b + 1]) {
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

void compare(const PointTables<PostTile> &T, const Brute &R, const std::vector<int64_t> &off, int Q, bool with_cov) {
    CHECK(T.tiles.size() == R.tiles.size() && T.chunks.size() == R.chunks.size() && T.work_need == R.work_need);
    std::vector<int> cover((size_t)off[kNb], 0);
    for (size_t k = 0; k < T.tiles.size(); k++) {
        const PostTile &a = T.tiles[k], &b = R.tiles[k];
        CHECK(a.e == b.e && a.p0 == b.p0 && a.cnt == b.cnt && a.pad == 0);
        CHECK(a.cnt >= 1 && a.cnt * Q <= 64 && a.p0 >= 0 && (int64_t)a.p0 + a.cnt <= off[kNb]);   // the columns of its points fit the tile
        for (int p = a.p0; p < a.p0 + a.cnt; p++) cover[p]++;
    }
    for (int v : cover) CHECK(v == 1);   // every point of the call in exactly one tile
    for (size_t k = 0; k < T.chunks.size(); k++) {
        const TileChunk &a = T.chunks[k], &b = R.chunks[k];
        CHECK(a.cls == b.cls && a.t0 == b.t0 && a.nt == b.nt && a.stride == b.stride);
        // the ld x 64 work rows, then one double per pair of the fullest tile: the kernel indexes pair e < cnt Q (Q - 1) / 2 there
        CHECK(a.stride >= (size_t)kCls[a.cls].ld * 64 + (with_cov ? (size_t)components_tw(Q) * Q * (Q - 1) / 2 : 0));
    }
}
}  // namespace

int main() {
    int cases = 0, cut = 0, over = 0;
    for (int Q : kQs) {
        const int P = components_tw(Q);
        CHECK(P >= 1 && P * Q <= 64 && (P + 1) * Q > 64);
        CHECK(components_extra(Q, true) == brute_extra(Q) && components_extra(Q, false) == 0);
        CHECK(components_extra(Q, true) <= 2016);
        // point counts on and around the tile width, and several tiles
        const int counts[7] = {0, 1, P - 1, P, P + 1, 2 * P + 1, 3 * P + 2};
        const int nc = 7;
        const size_t tile192 = ((size_t)192 * 64 + components_extra(Q, true)) * sizeof(double);
        const size_t tile64 = ((size_t)64 * 64 + components_extra(Q, true)) * sizeof(double);
        for (int rot = 0; rot < nc; rot++)
            for (int with_cov = 0; with_cov < 2; with_cov++)
                for (size_t budget : {(size_t)1 << 30, 3 * tile192, 3 * tile64, tile64, (size_t)1}) {
                    std::vector<int64_t> off(kNb + 1, 0);
                    for (int b = 0; b < kNb; b++) off[b + 1] = off[b] + counts[(b + rot) % nc];
                    PointTables<PostTile> T;
                    build_components_tiles(kCls, kOrder, off.data(), Q, with_cov != 0, budget, T);
                    const Brute R = brute(off, Q, with_cov != 0, budget);
                    compare(T, R, off, Q, with_cov != 0);
                    for (const TileChunk &ch : T.chunks) {
                        const size_t bytes = (size_t)ch.nt * ch.stride * sizeof(double);
                        CHECK(bytes <= budget || ch.nt == 1);
                        if (bytes > budget) over++;
                    }
                    if (T.chunks.size() > kCls.size()) cut++;
                    if (budget == (size_t)1) CHECK(T.chunks.size() == T.tiles.size());   // one tile per chunk
                    cases++;
                }
        // no point at all: no tile, no chunk, no work rows
        {
            const std::vector<int64_t> off(kNb + 1, 0);
            PointTables<PostTile> T;
            build_components_tiles(kCls, kOrder, off.data(), Q, true, tile64, T);
            CHECK(T.tiles.empty() && T.chunks.empty() && T.work_need == 0);
        }
    }
    // Q = 1 is the posterior call's table; the posterior call's builder is what it was
    {
        std::vector<int64_t> off(kNb + 1, 0);
        for (int b = 0; b < kNb; b++) off[b + 1] = off[b] + 200;
        PointTables<PostTile> P, T;
        build_point_tiles(kCls, kOrder, off.data(), nullptr, 0, (size_t)1 << 30, P);
        build_components_tiles(kCls, kOrder, off.data(), 1, true, (size_t)1 << 30, T);
        CHECK(P.tiles.size() == (size_t)kNb * 4 && T.tiles.size() == P.tiles.size() && T.work_need == P.work_need);
        for (size_t k = 0; k < P.tiles.size(); k++) CHECK(P.tiles[k].p0 == T.tiles[k].p0 && P.tiles[k].cnt == T.tiles[k].cnt);
    }
    CHECK(cut > 0 && over > 0);   // the budgets did cut chunks, and the one-byte budget did leave single tiles above it
    std::printf("components_tables ok: %d cases, %d with cut chunks\n", cases, cut);
    return 0;
}
