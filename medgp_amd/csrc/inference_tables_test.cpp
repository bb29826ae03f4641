// inference_tables_test.cpp -- CPU test of the table builders of inference_tables.h against brute-force restatements.
// Stand-alone (own main, no HIP): built with the host compiler and -fsanitize=address,undefined by tests/test_inference_tables.py, so an
// index mistake in the builders is caught here and not as an out-of-bounds access on a GPU.
#include "inference_tables.h"

#include <cstdio>
#include <cstdlib>
#include <numeric>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {
// the plan of every case: two size classes, largest first (ld = 192 with two entries, ld = 64 with three), a scrambled caller order
const std::vector<TableClass> kCls = {{0, 2, 192}, {2, 3, 64}};
const int kOrder[5] = {3, 0, 4, 1, 2};   // internal entry -> caller entry
const int kNb = 5;
const int kPointCounts[6] = {0, 1, 63, 64, 65, 200};
const size_t kTile192 = (size_t)192 * 64 * sizeof(double), kTile64 = (size_t)64 * 64 * sizeof(double);

int class_of(int i) { for (size_t k = 0; k < kCls.size(); k++) if (i >= kCls[k].b0 && i < kCls[k].b0 + kCls[k].count) return (int)k; CHECK(false); return -1; }
int internal_of(int b) { for (int i = 0; i < kNb; i++) if (kOrder[i] == b) return i; CHECK(false); return -1; }

// offsets of the case `rot`: caller entry b has kPointCounts[(b + rot) % 6] points
std::vector<int64_t> make_offsets(int rot) {
    std::vector<int64_t> off(kNb + 1, 0);
    for (int b = 0; b < kNb; b++) off[b + 1] = off[b] + kPointCounts[(b + rot) % 6];
    return off;
}
int patient_of_point(const std::vector<int64_t> &off, int64_t p) { for (int b = 0; b < kNb; b++) if (p >= off[b] && p < off[b + 1]) return b; CHECK(false); return -1; }

// every point in exactly one tile, no tile across two patients, tile.e / chunk.cls consistent; chunks partition the tiles in order,
// one class each, within the budget unless a single tile; work_need = the largest chunk; pmax = the largest prefix of the tile
template <class Tile>
void check_tiles(const PointTables<Tile> &T, const std::vector<int64_t> &off, size_t extra, size_t budget, const int *prefix, bool whole_patients) {
    std::vector<int> cover((size_t)off[kNb], 0);
    int next = 0;
    size_t need = 0;
    for (const TileChunk &ch : T.chunks) {
        CHECK(ch.t0 == next && ch.nt >= 1 && ch.cls >= 0 && ch.cls < (int)kCls.size());
        next += ch.nt;
        CHECK(ch.stride == (size_t)kCls[ch.cls].ld * 64 + extra);
        const size_t bytes = (size_t)ch.nt * ch.stride * sizeof(double);
        if (!whole_patients) CHECK(bytes <= budget || ch.nt == 1);
        need = std::max(need, bytes);
        for (int t = ch.t0; t < ch.t0 + ch.nt; t++) {
            const Tile &tl = T.tiles[t];
            CHECK(tl.cnt >= 1 && tl.cnt <= POST_TW && tl.p0 >= 0 && (int64_t)tl.p0 + tl.cnt <= off[kNb]);
            const int b = patient_of_point(off, tl.p0);
            CHECK((int64_t)tl.p0 + tl.cnt <= off[b + 1]);                      // no tile spans two patients
            CHECK(class_of(internal_of(b)) == ch.cls && tl.e == internal_of(b) - kCls[ch.cls].b0);
            int pm = 0;
            for (int p = tl.p0; p < tl.p0 + tl.cnt; p++) { cover[p]++; if (prefix) pm = std::max(pm, prefix[p]); }
            CHECK(reinterpret_cast<const int *>(&tl)[3] == pm);               // PostTile::pad = 0, ForeTile::pmax
        }
    }
    CHECK(next == (int)T.tiles.size() && need == T.work_need);
    for (int v : cover) CHECK(v == 1);
}

int test_point_tiles() {
    int cut = 0, over = 0;
    for (int rot = 0; rot < 6; rot++)
        for (size_t budget : {3 * kTile192, 3 * kTile64, (size_t)1})
            for (size_t extra : {(size_t)0, (size_t)40 * 64}) {
                const std::vector<int64_t> off = make_offsets(rot);
                PointTables<PostTile> P;
                build_point_tiles(kCls, kOrder, off.data(), nullptr, extra, budget, P);
                check_tiles(P, off, extra, budget, nullptr, false);
                // sorted prefixes inside every patient
                std::vector<int> prefix((size_t)off[kNb]);
                for (int b = 0; b < kNb; b++) for (int64_t p = off[b]; p < off[b + 1]; p++) prefix[p] = (int)((p - off[b]) * 7 / 3 + b);
                PointTables<ForeTile> F;
                build_point_tiles(kCls, kOrder, off.data(), prefix.data(), extra, budget, F);
                check_tiles(F, off, extra, budget, prefix.data(), false);
                CHECK(F.chunks.size() == P.chunks.size());
                if (P.chunks.size() > kCls.size()) cut++;
                for (const TileChunk &ch : P.chunks) if ((size_t)ch.nt * ch.stride * sizeof(double) > budget) over++;
            }
    CHECK(cut > 0 && over > 0);   // the budgets did cut chunks, and the one-byte budget did leave single tiles above it
    return cut;
}

size_t joint_need(int64_t m, int ld, size_t extra, bool want_cov) {
    const size_t nt = (size_t)((m + 63) / 64), mpad = nt * 64;
    return nt * ((size_t)ld * 64 + extra) * 8 + mpad * mpad * 8 + (want_cov ? (size_t)m * m * 4 : 0);
}

void test_joint(int *n_ok, int *n_cut, int *n_err) {
    for (int rot = 0; rot < 6; rot++)
        for (size_t budget : {3 * kTile192, (size_t)700000, (size_t)4 << 20})
            for (int want_cov = 0; want_cov < 2; want_cov++) {
                const std::vector<int64_t> off = make_offsets(rot);
                int first_bad = -1;   // the first patient (internal order) that alone exceeds the budget
                for (int i = 0; i < kNb && first_bad < 0; i++) {
                    const int b = kOrder[i];
                    if (off[b + 1] > off[b] && joint_need(off[b + 1] - off[b], kCls[class_of(i)].ld, 0, want_cov) > budget) first_bad = i;
                }
                JointTables T;
                TableError e{-1, -1, -1, 0, 0};
                const bool ok = build_joint_chunks(kCls, kOrder, off.data(), 0, want_cov != 0, budget, T, e);
                CHECK(ok == (first_bad < 0));
                if (!ok) {
                    CHECK(e.entry == first_bad && e.b == kOrder[first_bad] && e.m == off[e.b + 1] - off[e.b]);
                    CHECK(e.need == joint_need(e.m, kCls[class_of(first_bad)].ld, 0, want_cov) && e.need > budget);
                    (*n_err)++;
                    continue;
                }
                (*n_ok)++;
                check_tiles(T, off, 0, budget, nullptr, true);
                std::vector<int> seen(kNb, 0);
                int npat = 0, npair = 0, nblk = 0;
                size_t wneed = 0, cneed = 0, vneed = 0;
                for (const TileChunk &ch : T.chunks) {
                    CHECK(ch.pat0 == npat && ch.pair0 == npair && ch.blk0 == nblk && ch.npat >= 1);
                    int tile = 0;
                    size_t cd = 0, cf = 0;
                    std::vector<std::pair<long long, long long>> cr, vr;   // [begin, end) of every patient's C / cov block
                    for (int p = ch.pat0; p < ch.pat0 + ch.npat; p++) {
                        const JointPat &J = T.pats[p];
                        CHECK(J.b >= 0 && J.b < kNb && !seen[J.b]++);
                        const int i = internal_of(J.b), nt = (J.m + 63) / 64;
                        CHECK(J.m == off[J.b + 1] - off[J.b] && J.m > 0 && J.p0 == off[J.b] && class_of(i) == ch.cls && J.e == i - kCls[ch.cls].b0);
                        // cut only at patient boundaries: the patient's tiles are the chunk's next nt tiles, all its own
                        CHECK(J.tile0 == tile);
                        for (int t = 0; t < nt; t++) { const PostTile &tl = T.tiles[ch.t0 + tile + t]; CHECK(tl.e == J.e && tl.p0 == J.p0 + 64 * t); }
                        tile += nt;
                        int pairs = 0, blks = 0;
                        std::vector<int> hit((size_t)nt * nt, 0);
                        for (int q = ch.pair0; q < ch.pair0 + ch.npair; q++)
                            if (T.pairs[q].pat == p) { const JointTile &t = T.pairs[q]; CHECK(t.I >= t.J && t.J >= 0 && t.I < nt && !hit[t.I * nt + t.J]++); pairs++; }
                        for (int q = ch.blk0; q < ch.blk0 + ch.nblk; q++)
                            if (T.blks[q].pat == p) { CHECK(T.blks[q].I == blks); blks++; }
                        CHECK(pairs == nt * (nt + 1) / 2 && blks == nt);
                        const long long mpad = 64LL * nt;
                        cr.push_back({J.coff, J.coff + mpad * mpad});
                        vr.push_back({J.voff, J.voff + (want_cov ? (long long)J.m * J.m : 0)});
                        cd = std::max<size_t>(cd, (size_t)cr.back().second); cf = std::max<size_t>(cf, (size_t)vr.back().second);
                    }
                    CHECK(tile == ch.nt);
                    for (size_t a = 0; a < cr.size(); a++)
                        for (size_t z = a + 1; z < cr.size(); z++) {
                            CHECK(cr[a].first >= 0 && (cr[a].second <= cr[z].first || cr[z].second <= cr[a].first));
                            CHECK(vr[a].first >= 0 && (vr[a].second <= vr[z].first || vr[z].second <= vr[a].first));
                        }
                    const size_t wb = (size_t)ch.nt * ch.stride * 8;
                    CHECK(wb + cd * 8 + cf * 4 <= budget);
                    CHECK(cd * 8 <= T.c_need && cf * 4 <= T.cov_need && wb <= T.work_need);
                    wneed = std::max(wneed, wb); cneed = std::max(cneed, cd * 8); vneed = std::max(vneed, cf * 4);
                    npat += ch.npat; npair += ch.npair; nblk += ch.nblk;
                }
                CHECK(npat == (int)T.pats.size() && npair == (int)T.pairs.size() && nblk == (int)T.blks.size());
                CHECK(wneed == T.work_need && cneed == T.c_need && vneed == T.cov_need);
                for (int b = 0; b < kNb; b++) CHECK(seen[b] == (off[b + 1] > off[b] ? 1 : 0));
                if (T.chunks.size() > kCls.size()) (*n_cut)++;
            }
}

void test_loo(int *n_ok, int *n_cut, int *n_err) {
    // sizes of the internal entries (two of 64 < n <= 192, three of n <= 64) and group ids per caller entry: -1 (never held out), empty
    // groups, singletons, a 130-member group; two patients not uploaded grouped (a permutation internal row -> caller observation)
    const int en[5] = {190, 150, 64, 40, 7};
    std::vector<int64_t> ooff(kNb + 1, 0), goff(kNb + 1, 0);
    std::vector<int> nobs(kNb), ng(kNb);
    for (int i = 0; i < kNb; i++) nobs[kOrder[i]] = en[i];
    for (int b = 0; b < kNb; b++) { ng[b] = 9; ooff[b + 1] = ooff[b] + nobs[b]; goff[b + 1] = goff[b] + ng[b]; }
    std::vector<int32_t> group((size_t)ooff[kNb]);
    for (int b = 0; b < kNb; b++)
        for (int o = 0; o < nobs[b]; o++) {
            // 190 observations: group 0 = 130 members (o % 19 < 13), group 1 empty, group 2 a singleton, groups 3 .. 6 of 10 - 16, -1 the rest
            int g = (o % 19 < 13) ? 0 : (o == 13 ? 2 : (o % 19 < 17 ? 3 + (o / 19) % 4 : -1));
            if (nobs[b] == 7) g = o < 5 ? o + 3 : -1;   // singletons only
            group[ooff[b] + o] = g;
        }
    std::vector<std::vector<int>> perms(kNb);
    std::vector<const int *> perm(kNb, nullptr);
    for (int b : {kOrder[0], kOrder[3]}) {
        perms[b].resize(nobs[b]);
        for (int r = 0; r < nobs[b]; r++) perms[b][r] = (int)(((long long)r * 7 + 3) % nobs[b]);   // (7 is coprime to 190 and 40)
        perm[b] = perms[b].data();
    }
    for (int use_groups = 0; use_groups < 2; use_groups++)
        for (size_t budget : {3 * kTile192, (size_t)700000, (size_t)4 << 20})
            for (int flags = 0; flags < 4; flags++) {
                const bool want_var = flags & 1, want_vec = flags & 2;
                std::vector<int64_t> go = goff;
                if (!use_groups) for (int b = 0; b < kNb; b++) go[b + 1] = go[b] + nobs[b];   // every observation its own group
                // brute force: members of every group, in caller observations
                std::vector<std::vector<int>> mem((size_t)go[kNb]);
                for (int b = 0; b < kNb; b++)
                    for (int o = 0; o < nobs[b]; o++) { const int g = use_groups ? group[ooff[b] + o] : o; if (g >= 0) mem[go[b] + g].push_back((int)ooff[b] + o); }
                bool fits = true;
                for (const auto &m : mem) if (m.size() >= 2 && loo_block_doubles((int)m.size()) * 8 > budget) fits = false;
                LooTables T;
                TableError e{-1, -1, -1, 0, 0};
                const bool ok = build_loo_tables(kCls, kOrder, en, ooff.data(), go.data(), kNb, use_groups ? group.data() : nullptr, perm.data(), want_var, want_vec, budget, T, e);
                CHECK(ok == fits);
                if (!ok) {
                    CHECK(e.b >= 0 && e.b < kNb && e.gid >= 0 && e.m == (long long)mem[go[e.b] + e.gid].size() && e.need == loo_block_doubles((int)e.m) * 8 && e.need > budget);
                    (*n_err)++;
                    continue;
                }
                (*n_ok)++;
                CHECK(T.gsize.size() == mem.size());
                for (size_t g = 0; g < mem.size(); g++) CHECK(T.gsize[g] == (int)mem[g].size());
                // every held-out observation in exactly one of singles and rows
                std::vector<int> held((size_t)ooff[kNb], 0);
                auto row_of = [&](int b, int r) { return (int)ooff[b] + (perm[b] ? perm[b][r] : r); };   // caller observation of internal row r
                CHECK(T.csing.size() == kCls.size());
                int snext = 0;
                for (const LooClassSingles &cs : T.csing) {
                    CHECK(cs.s0 == snext && cs.ns >= 0);
                    snext += cs.ns;
                    for (int s = cs.s0; s < cs.s0 + cs.ns; s++) {
                        const LooSingle &S = T.singles[s];
                        CHECK(S.e >= 0 && S.e < kCls[cs.cls].count);
                        const int i = kCls[cs.cls].b0 + S.e, b = kOrder[i];
                        CHECK(S.r >= 0 && S.r < en[i] && S.out == row_of(b, S.r) && S.g >= go[b] && S.g < go[b + 1]);
                        CHECK(mem[S.g].size() == 1 && mem[S.g][0] == S.out);
                        held[S.out]++;
                    }
                }
                CHECK(snext == (int)T.singles.size());
                int gnext = 0, pnext = 0, jnext = 0, rnext = 0;
                size_t need = 0;
                for (const LooChunk &ch : T.chunks) {
                    CHECK(ch.g0 == gnext && ch.pair0 == pnext && ch.job0 == jnext && ch.ng >= 1);
                    size_t end = 0;
                    std::vector<std::pair<long long, long long>> blk;
                    for (int g = ch.g0; g < ch.g0 + ch.ng; g++) {
                        const JointPat &G = T.groups[g];
                        CHECK(G.e >= 0 && G.e < kCls[ch.cls].count);
                        const int i = kCls[ch.cls].b0 + G.e, b = kOrder[i], nt = (G.m + 63) / 64;
                        CHECK(G.b >= go[b] && G.b < go[b + 1] && G.m == (int)mem[G.b].size() && G.m >= 2 && G.p0 == rnext);
                        rnext += G.m;
                        for (int k = 0; k < G.m; k++) {   // its rows: ascending, its own members
                            const LooRow &R = T.rows[G.p0 + k];
                            CHECK(R.r >= 0 && R.r < en[i] && R.out == row_of(b, R.r) && (k == 0 || R.r > T.rows[G.p0 + k - 1].r));
                            CHECK(std::find(mem[G.b].begin(), mem[G.b].end(), R.out) != mem[G.b].end());
                            held[R.out]++;
                        }
                        int pairs = 0, col = 0, vec = 0;
                        for (int q = ch.pair0; q < ch.pair0 + ch.npair; q++) if (T.pairs[q].pat == g) { CHECK(T.pairs[q].I >= T.pairs[q].J && T.pairs[q].I < nt && T.pairs[q].J >= 0); pairs++; }
                        for (int q = ch.job0; q < ch.job0 + ch.njob; q++)
                            if (T.jobs[q].pat == g) { if (T.jobs[q].J == 1) { CHECK(T.jobs[q].I == 0); vec++; } else { CHECK(T.jobs[q].J == 0 && T.jobs[q].I == col); col++; } }
                        CHECK(pairs == nt * (nt + 1) / 2 && col == (want_var ? nt : 0) && vec == (want_vec ? 1 : 0));
                        blk.push_back({G.coff, G.coff + (long long)loo_block_doubles(G.m)});
                        end = std::max(end, (size_t)blk.back().second);
                    }
                    for (size_t a = 0; a < blk.size(); a++)
                        for (size_t z = a + 1; z < blk.size(); z++) CHECK(blk[a].first >= 0 && (blk[a].second <= blk[z].first || blk[z].second <= blk[a].first));
                    CHECK(end * 8 <= budget && end * 8 <= T.blk_need);
                    need = std::max(need, end * 8);
                    gnext += ch.ng; pnext += ch.npair; jnext += ch.njob;
                }
                CHECK(gnext == (int)T.groups.size() && pnext == (int)T.pairs.size() && jnext == (int)T.jobs.size() && rnext == (int)T.rows.size() && need == T.blk_need);
                for (int b = 0; b < kNb; b++)
                    for (int o = 0; o < nobs[b]; o++) CHECK(held[ooff[b] + o] == ((use_groups ? group[ooff[b] + o] : o) >= 0 ? 1 : 0));
                int nclass_with_groups = 0;
                for (size_t k = 0; k < kCls.size(); k++) { bool any = false; for (const LooChunk &ch : T.chunks) any = any || ch.cls == (int)k; nclass_with_groups += any; }
                if ((int)T.chunks.size() > nclass_with_groups) (*n_cut)++;
            }
}
}  // namespace

int main() {
    const int pcut = test_point_tiles();
    int jok = 0, jcut = 0, jerr = 0, lok = 0, lcut = 0, lerr = 0;
    test_joint(&jok, &jcut, &jerr);
    test_loo(&lok, &lcut, &lerr);
    // every branch was met: chunks were cut, and one joint patient / one LOO group exceeded the budget
    CHECK(jok > 0 && jcut > 0 && jerr > 0 && lok > 0 && lcut > 0 && lerr > 0);
    std::printf("inference_tables ok: point cases cut %d; joint ok %d cut %d over-budget %d; loo ok %d cut %d over-budget %d\n", pcut, jok, jcut, jerr, lok, lcut, lerr);
    return 0;
}
