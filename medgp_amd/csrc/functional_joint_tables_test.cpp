// functional_joint_tables_test.cpp -- CPU test of the chunk builder of medgp_functional_joint_batch (build_functional_joint_chunks,
// inference_tables.h) against a brute-force restatement: functional counts per patient on and around the tile width and over several
// tiles, budgets from "everything in one chunk" to "one patient per chunk", the patient that alone exceeds the budget; every patient
// with functionals appears once, every lower tile pair of it once, the tiles are those of build_functional_tiles, and every offset
// stays inside the needs the entry point allocates.  Stand-alone (own main, no HIP): built with the host compiler and
// -fsanitize=address,undefined by tests/test_functional_joint_tables.py, so an index mistake is caught here and not as an
// out-of-bounds access on a GPU.
#include "inference_tables.h"

#include <cstdio>
#include <cstdlib>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {
const int kNb = 7;
struct Setup { std::vector<TableClass> cls; int order[kNb]; };   // order: internal entry -> caller entry
// two size classes, largest first (ld = 192 with three entries, ld = 64 with four), a scrambled caller order
const Setup kTwo = {{{0, 3, 192}, {3, 4, 64}}, {3, 0, 6, 4, 1, 5, 2}};
// one size class: every patient has the same bytes per tile
const Setup kOne = {{{0, 7, 64}}, {6, 5, 4, 3, 2, 1, 0}};
const int kCounts[7] = {0, 1, 63, 64, 65, 130, 200};

// bytes of one patient: the work rows of its tiles and its F x F floats
size_t need_of(int64_t F, int ld) { return (size_t)((F + 63) / 64) * (size_t)ld * 64 * 8 + (size_t)F * (size_t)F * 4; }

struct BrutePat { int i, b, cls, chunk; int64_t F; };
// brute force: walk the classes and their internal entries; a patient with functionals joins the open chunk of its class if the
// chunk's bytes with it stay within the budget, and opens a new one otherwise; a class ends its chunk
bool brute(const Setup &S, const std::vector<int64_t> &foff, size_t budget, std::vector<BrutePat> &pats, int *nchunks, int *first_bad) {
    pats.clear();
    *nchunks = 0;
    *first_bad = -1;
    const std::vector<TableClass> &kCls = S.cls;
    for (int ci = 0; ci < (int)kCls.size(); ci++) {
        size_t bytes = 0;
        bool open = false;
        for (int i = kCls[ci].b0; i < kCls[ci].b0 + kCls[ci].count; i++) {
            const int b = S.order[i];
            const int64_t F = foff[b + 1] - foff[b];
            if (F == 0) continue;
            const size_t need = need_of(F, kCls[ci].ld);
            if (need > budget) { *first_bad = i; return false; }
            if (!open || bytes + need > budget) { (*nchunks)++; bytes = 0; open = true; }
            bytes += need;
            pats.push_back({i, b, ci, *nchunks - 1, F});
        }
    }
    return true;
}

int n_ok = 0, n_cut = 0, n_err = 0, n_single = 0;
void run(const Setup &S, const std::vector<int64_t> &foff, size_t budget);
}  // namespace

int main() {
    const size_t largest = need_of(200, 192), all = kNb * largest;
    // budgets: everything in one chunk per class; a few patients per chunk; exactly the largest patient of any rotation (one or two
    // patients per chunk); just below it (the over-budget patient); tiny
    const size_t budgets[] = {all, need_of(200, 192) + need_of(130, 192), need_of(130, 64) + need_of(65, 64) + 1, largest, largest - 1,
                              need_of(65, 192), need_of(1, 64), 1};
    for (int rot = 0; rot < kNb; rot++)
        for (size_t budget : budgets) {
            std::vector<int64_t> foff(kNb + 1, 0);
            for (int b = 0; b < kNb; b++) foff[b + 1] = foff[b] + kCounts[(b + rot) % kNb];
            run(kTwo, foff, budget);
            run(kOne, foff, budget);
        }
    // one patient per chunk: equal patients, a budget one byte short of two of them
    for (int F : {1, 64, 65, 130}) {
        std::vector<int64_t> foff(kNb + 1, 0);
        for (int b = 0; b < kNb; b++) foff[b + 1] = foff[b] + F;
        const int before = n_single;
        run(kOne, foff, 2 * need_of(F, 64) - 1);
        CHECK(n_single == before + 1);
        run(kOne, foff, 2 * need_of(F, 64));   // and two per chunk
        CHECK(n_single == before + 1);
    }
    // no functional at all: no tile, no patient, no chunk
    {
        const std::vector<int64_t> foff(kNb + 1, 0);
        JointTables T;
        TableError e{-1, -1, -1, 0, 0};
        CHECK(build_functional_joint_chunks(kTwo.cls, kTwo.order, foff.data(), 1, T, e));
        CHECK(T.tiles.empty() && T.pats.empty() && T.pairs.empty() && T.chunks.empty() && T.work_need == 0 && T.cov_need == 0);
    }
    // the largest count the interface admits does not overflow the byte count: it is reported as over the budget
    {
        const std::vector<TableClass> cls = {{0, 1, 64}};
        const int order[1] = {0};
        const int64_t foff[2] = {0, FUNC_MAX_FUNCTIONALS};
        JointTables T;
        TableError e{-1, -1, -1, 0, 0};
        CHECK(!build_functional_joint_chunks(cls, order, foff, (size_t)1 << 40, T, e));
        CHECK(e.b == 0 && e.m == FUNC_MAX_FUNCTIONALS && T.pats.empty());
    }
    CHECK(n_ok > 0 && n_cut > 0 && n_err > 0 && n_single > 0);
    std::printf("functional_joint_tables ok: %d cases, %d with cut chunks, %d with one patient per chunk, %d over the budget\n", n_ok, n_cut, n_single, n_err);
    return 0;
}

namespace {
void run(const Setup &S, const std::vector<int64_t> &foff, size_t budget) {
    const std::vector<TableClass> &kCls = S.cls;
    const int64_t F = foff[kNb];
    std::vector<BrutePat> bp;
    int bchunks = 0, first_bad = -1;
    const bool bok = brute(S, foff, budget, bp, &bchunks, &first_bad);
    JointTables T;
    TableError e{-1, -1, -1, 0, 0};
    const bool ok = build_functional_joint_chunks(kCls, S.order, foff.data(), budget, T, e);
    CHECK(ok == bok);
    if (!ok) {
        const int cls_of = (kCls.size() > 1 && first_bad >= kCls[1].b0) ? 1 : 0;
        CHECK(e.entry == first_bad && e.b == S.order[first_bad] && e.gid == -1 && e.m == foff[e.b + 1] - foff[e.b]);
        CHECK(e.need == need_of(e.m, kCls[cls_of].ld) && e.need > budget);
        n_err++;
        return;
    }
    n_ok++;
    // the tiles are those of the per-functional call, in its order (k_functional_prep and k_functional read the same table)
    PointTables<PostTile> P;
    build_functional_tiles(kCls, S.order, foff.data(), (size_t)1 << 40, P);
    CHECK(T.tiles.size() == P.tiles.size());
    for (size_t k = 0; k < T.tiles.size(); k++) {
        const PostTile &a = T.tiles[k], &b = P.tiles[k];
        CHECK(a.e == b.e && a.p0 == b.p0 && a.cnt == b.cnt && a.pad == 0 && a.cnt >= 1 && a.cnt <= FUNC_TW && (int64_t)a.p0 + a.cnt <= F);
    }
    CHECK(T.blks.empty() && T.c_need == 0);   // no row blocks, no fp64 C: nothing is factored
    CHECK(T.pats.size() == bp.size() && (int)T.chunks.size() == bchunks);
    std::vector<int> seen(kNb, 0);
    int npat = 0, npair = 0, ntile = 0;
    size_t wneed = 0, vneed = 0;
    for (size_t c = 0; c < T.chunks.size(); c++) {
        const TileChunk &ch = T.chunks[c];
        CHECK(ch.pat0 == npat && ch.pair0 == npair && ch.t0 == ntile && ch.npat >= 1 && ch.nblk == 0 && ch.stride == (size_t)kCls[ch.cls].ld * 64);
        if (c > 0) CHECK(T.chunks[c - 1].cls <= ch.cls);   // the chunks of a class are consecutive (one k_functional_prep launch per class)
        int tile = 0, pairs_in_chunk = 0;
        size_t cf = 0;
        std::vector<std::pair<long long, long long>> vr;   // [begin, end) of every patient's block of the chunk's cov buffer
        for (int p = ch.pat0; p < ch.pat0 + ch.npat; p++) {
            const JointPat &J = T.pats[p];
            const BrutePat &R = bp[(size_t)p];
            CHECK(J.b >= 0 && J.b < kNb && !seen[J.b]++);   // every patient once
            CHECK(J.b == R.b && R.chunk == (int)c && R.cls == ch.cls && J.e == R.i - kCls[ch.cls].b0);
            CHECK(J.m == R.F && J.m > 0 && J.p0 == foff[J.b] && J.coff == 0 && J.pad == 0);
            const int nt = (J.m + 63) / 64;
            // cut only at patient boundaries: the patient's tiles are the chunk's next nt tiles, all its own
            CHECK(J.tile0 == tile);
            for (int t = 0; t < nt; t++) {
                const PostTile &tl = T.tiles[(size_t)(ch.t0 + tile + t)];
                CHECK(tl.e == J.e && tl.p0 == J.p0 + 64 * t && tl.cnt == std::min(64, J.m - 64 * t));
            }
            tile += nt;
            int pairs = 0;
            std::vector<int> hit((size_t)nt * nt, 0);
            for (int q = ch.pair0; q < ch.pair0 + ch.npair; q++)
                if (T.pairs[(size_t)q].pat == p) {
                    const JointTile &t = T.pairs[(size_t)q];
                    CHECK(t.I >= t.J && t.J >= 0 && t.I < nt && !hit[(size_t)(t.I * nt + t.J)]++);   // every lower pair once
                    pairs++;
                }
            CHECK(pairs == nt * (nt + 1) / 2);
            pairs_in_chunk += pairs;
            vr.push_back({J.voff, J.voff + (long long)J.m * J.m});
            cf = std::max<size_t>(cf, (size_t)vr.back().second);
        }
        CHECK(tile == ch.nt && pairs_in_chunk == ch.npair);   // no pair of another chunk's patient
        for (size_t a = 0; a < vr.size(); a++) {
            CHECK(vr[a].first >= 0);
            for (size_t z = a + 1; z < vr.size(); z++) CHECK(vr[a].second <= vr[z].first || vr[z].second <= vr[a].first);
        }
        const size_t wb = (size_t)ch.nt * ch.stride * 8;
        CHECK(wb + cf * 4 <= budget);
        CHECK(cf * 4 <= T.cov_need && wb <= T.work_need);   // offsets stay inside the needs
        wneed = std::max(wneed, wb); vneed = std::max(vneed, cf * 4);
        npat += ch.npat; npair += ch.npair; ntile += ch.nt;
    }
    CHECK(npat == (int)T.pats.size() && npair == (int)T.pairs.size() && ntile == (int)T.tiles.size());
    CHECK(wneed == T.work_need && vneed == T.cov_need);   // and the needs are no larger than the largest chunk
    for (int b = 0; b < kNb; b++) CHECK(seen[b] == (foff[b + 1] > foff[b] ? 1 : 0));
    if (T.chunks.size() > kCls.size()) n_cut++;
    if (T.chunks.size() == T.pats.size()) n_single++;
}
}  // namespace
