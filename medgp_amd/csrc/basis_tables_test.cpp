// basis_tables_test.cpp -- CPU test of basis_tables.h: the resident store of medgp_set_basis (placement in place / appended /
// compacted into a new block, the row map into the grouped order) and every address k_basis_g and k_basis_post touch through the
// element maps (the loops below restate the kernels' index ranges over the same maps).  Stand-alone (own main, no HIP): built with the
// host compiler and -fsanitize=address,undefined by tests/test_basis_truth.py, so an index mistake shows here and not as an
// out-of-bounds access on a GPU.  The buffers are real allocations of the computed sizes: the sanitizer checks the bounds, the counts
// that every element of G of an entry's own blocks is written exactly once and that everything read was written.
// Build and run: make basis_tables_test && ./basis_tables_test
#include "basis_tables.h"
#include "call_plan.h"
#include "pjvp_tables.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

unsigned g_seed = 12345;
int rnd(int m) { g_seed = g_seed * 1664525u + 1013904223u; return (int)((g_seed >> 8) % (unsigned)m); }

// a value that names (slot, version, caller row, column)
double tag(int slot, int ver, int row, int col) { return ((slot * 131.0 + ver) * 1024.0 + row) * 64.0 + col; }

// the host's side of medgp_set_basis against a real block: returns the block after the call
struct Sim {
    BasisStore st;
    std::vector<double> blk;
    std::vector<int> ver, n;                  // per slot: version of the basis it carries (-1: none), rows
    std::vector<std::vector<int>> perm;       // internal row -> caller row
    int grown = 0, in_place = 0;

    void set(const std::vector<int32_t> &slots, int p) {
        std::vector<int> rows;
        size_t total = 0;
        for (int s : slots) { rows.push_back(n[s]); total += BasisStore::need(n[s], p); }
        const size_t used_before = st.used;
        const BasisPlace pl = st.place((int)slots.size(), slots.data(), rows.data(), p);
        if (pl.new_cap) {
            std::vector<double> nb(pl.new_cap, -1.0);
            for (const BasisMove &m : pl.moves) {
                CHECK(m.src + m.count <= blk.size() && m.dst + m.count <= nb.size());
                std::copy(blk.begin() + m.src, blk.begin() + m.src + m.count, nb.begin() + m.dst);
            }
            blk.swap(nb);
            grown++;
        } else if (pl.moves.empty() && st.used == used_before && total) in_place++;
        CHECK(st.cap == blk.size() && st.used <= st.cap && pl.base + total <= blk.size());
        std::vector<double> stage(total ? total : 1), caller;
        size_t at = 0;
        for (int s : slots) {
            ver[s]++;
            caller.assign(BasisStore::need(n[s], p) + 1, 0.0);
            for (int i = 0; i < n[s]; i++)
                for (int c = 0; c < p; c++) caller[basis_h_at(i, p, c)] = tag(s, ver[s], i, c);
            basis_pack_rows(caller.data(), perm[s].data(), n[s], p, stage.data() + at);
            at += BasisStore::need(n[s], p);
        }
        std::copy(stage.begin(), stage.begin() + total, blk.begin() + pl.base);   // the ONE transfer
        at = pl.base;
        for (int s : slots) { CHECK(st.slot[s].off == (long long)at && st.slot[s].p == p && st.slot[s].rows == n[s]); at += BasisStore::need(n[s], p); }
    }
    // every live slot's range is inside the block, disjoint from the others and holds its own rows in the grouped order
    void verify() const {
        std::vector<char> owner(blk.size(), 0);
        for (int s = 0; s < (int)st.slot.size(); s++) {
            if (!st.has(s)) continue;
            const BasisSlot &b = st.slot[s];
            CHECK(b.rows == n[s] && (size_t)b.off + BasisStore::need(b.rows, b.p) <= st.used);
            for (int i = 0; i < b.rows; i++)
                for (int c = 0; c < b.p; c++) {
                    const size_t at = (size_t)b.off + basis_h_at(i, b.p, c);
                    CHECK(owner[at]++ == 0);
                    CHECK(blk[at] == tag(s, ver[s], perm[s][i], c));
                }
        }
    }
};

void store_walk() {
    const int S = 12;
    Sim sim;
    sim.st.slot.assign(S, BasisSlot{});
    sim.ver.assign(S, -1);
    sim.n.resize(S);
    sim.perm.resize(S);
    auto new_patient = [&](int s) {
        sim.n[s] = 3 + rnd(200);
        sim.perm[s].resize(sim.n[s]);
        std::iota(sim.perm[s].begin(), sim.perm[s].end(), 0);
        if (s % 2)   // an interleaved upload: a stable grouping by (row mod 3), as the library groups by covariate
            std::stable_sort(sim.perm[s].begin(), sim.perm[s].end(), [](int a, int b) { return a % 3 < b % 3; });
        std::vector<char> seen(sim.n[s], 0);   // a permutation
        for (int v : sim.perm[s]) { CHECK(v >= 0 && v < sim.n[s] && !seen[v]); seen[v] = 1; }
        sim.st.drop(s);
    };
    for (int s = 0; s < S; s++) new_patient(s);
    const int ps[] = {1, 2, 16, 17, 33, 64};
    std::vector<int32_t> all(S);
    std::iota(all.begin(), all.end(), 0);
    sim.set(all, 24);
    sim.verify();
    const int before = sim.in_place;
    sim.set(all, 24);   // the training loop's repeat: in place
    CHECK(sim.in_place == before + 1 && sim.grown == 1);
    sim.verify();
    for (int step = 0; step < 400; step++) {
        const int kind = rnd(10);
        if (kind == 0) { new_patient(rnd(S)); sim.verify(); continue; }
        if (kind == 1) { sim.st.drop(rnd(S)); sim.verify(); continue; }
        std::vector<int32_t> sl;
        for (int s = 0; s < S; s++) if (rnd(3) == 0) sl.push_back(s);
        if (sl.empty()) sl.push_back(rnd(S));
        if (rnd(2)) std::reverse(sl.begin(), sl.end());
        sim.set(sl, ps[rnd(6)]);
        sim.verify();
    }
    CHECK(sim.grown >= 3 && sim.in_place >= 1);
    std::printf("  store: %d blocks, %d calls in place, %zu of %zu doubles in use\n", sim.grown, sim.in_place, sim.st.used, sim.st.cap);
}

// en: observations per caller entry, mpts: test points per caller entry; p columns
int run_call(const std::vector<int> &en_caller, const std::vector<int> &mpts, int p, size_t post_budget) {
    const int nbatch = (int)en_caller.size();
    PlanRules r;
    r.Q = 5; r.D = 3; r.max_batch = nbatch; r.mem_budget = (size_t)64 << 20;
    BatchPlan P;
    layout_plan(r, en_caller.data(), nbatch, true, P);
    CHECK(P.nwaves == 1 && mean_fits(P.need_mat, P.need_vec, r.mem_budget));
    const MeanBuffers mb = mean_buffers(P.need_vec, nbatch, p);
    // the resident bases of the call's slots (slot = caller entry), offsets in the caller's order
    BasisStore st;
    st.slot.assign(nbatch, BasisSlot{});
    std::vector<int32_t> sl(nbatch);
    std::iota(sl.begin(), sl.end(), 0);
    const BasisPlace pl = st.place(nbatch, sl.data(), en_caller.data(), p);
    CHECK(pl.new_cap >= st.used && pl.base == 0);
    std::vector<char> Hs(pl.new_cap, 0), G(mb.panel_doubles, 0), U(P.need_mat, 0);
    for (int b = 0; b < nbatch; b++)   // the upload
        for (size_t x = 0; x < BasisStore::need(en_caller[b], p); x++) Hs[(size_t)st.slot[b].off + x]++;
    for (const SizeClass &k : P.cls) {
        char *Gk = G.data() + MEAN_PW * k.off_vec, *Uk = U.data() + k.off_mat;
        const int ld = k.ld;
        // k_basis_g: grid (basis_g_grid(nbmax), count); per step the staging rows r = w, w + 4, ..., lane = column of the block
        for (int b = 0; b < k.count; b++)
            for (int I = 0; I < basis_g_grid(k.nbmax); I++) {
                const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64, pos = P.order[(size_t)k.b0 + b];
                if (64 * I >= npad) continue;
                CHECK(en_caller[pos] == n && basis_g_kend(I) <= npad && basis_g_kend(I) % BASIS_KC == 0);
                const char *H = Hs.data() + st.slot[pos].off;
                for (int k0 = 0; k0 < basis_g_kend(I); k0 += BASIS_KC)
                    for (int w = 0; w < 4; w++) {
                        for (int rr = w; rr < BASIS_KC; rr += 4)
                            for (int lane = 0; lane < 64; lane++) {
                                const int j = k0 + rr, i = 64 * I + lane;
                                CHECK(rr < BASIS_KC && lane < BASIS_LDS_STRIDE);
                                if (j <= i && i < n) Uk[(size_t)b * ld * ld + (size_t)j * ld + i] = 1;
                                if (j < n && lane < p) CHECK(H[basis_h_at(j, p, lane)] == 1);
                            }
                        // a skipped step holds nothing of this wave's rows inside the triangle
                        if (k0 > basis_g_wave_klast(I, w)) CHECK(k0 > 64 * I + 16 * w + 15);
                        for (int kk = 0; kk < BASIS_KC; kk += 4)
                            for (int g = 0; g < 4; g++) CHECK(kk + g < BASIS_KC && 16 * w + 15 < BASIS_LDS_STRIDE);
                    }
                for (int rl = 0; rl < 64; rl++)
                    for (int col = 0; col < MEAN_PW; col++) Gk[mean_panel_at(b, ld, 64 * I + rl, col)]++;
            }
    }
    for (const SizeClass &k : P.cls)
        for (int b = 0; b < k.count; b++) {
            const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64;
            for (int i = 0; i < k.ld; i++)
                for (int col = 0; col < MEAN_PW; col++) CHECK(G[MEAN_PW * k.off_vec + mean_panel_at(b, k.ld, i, col)] == (i < npad ? 1 : 0));
        }
    // the posterior: pjvp_tables.h's tiles and chunks; k_basis_post reads V, G (rows < npad, the column tiles below p) and the
    // tile's rows of h2
    std::vector<int64_t> offsets(nbatch + 1, 0);
    for (int b = 0; b < nbatch; b++) offsets[b + 1] = offsets[b] + mpts[b];
    const int64_t M = offsets[nbatch];
    std::vector<TableClass> cls;
    for (const SizeClass &k : P.cls) cls.push_back({k.b0, k.count, k.ld});
    PointTables<PostTile> T;
    build_pjvp_tiles(cls, P.order.data(), offsets.data(), post_budget, T);
    const size_t Mz = (size_t)(M > 0 ? M : 1);
    std::vector<char> out(2 * Mz, 0), h2((size_t)M * p + 1, 1), h2read((size_t)M * p + 1, 0);
    for (const TileChunk &ch : T.chunks) {
        const SizeClass &k = P.cls[ch.cls];
        for (int x = 0; x < ch.nt; x++) {
            const PostTile &t = T.tiles[(size_t)ch.t0 + x];
            CHECK(t.e >= 0 && t.e < k.count && t.cnt >= 1 && t.cnt <= POST_TW);
            const int n = P.en[(size_t)k.b0 + t.e], npad = (n + 63) / 64 * 64;
            for (int kk = 0; kk < npad; kk++)
                for (int d = 0; d < 16 * ((p + 15) / 16); d++) CHECK(G[MEAN_PW * k.off_vec + mean_panel_at(t.e, k.ld, kk, d)] == 1);
            for (int j = 0; j < t.cnt; j++) {
                const size_t pt = (size_t)t.p0 + j;
                for (int d = 0; d < p; d++) { CHECK(h2[pt * p + d] == 1); h2read[pt * p + d]++; }
                out[pt]++; out[Mz + pt]++;
            }
        }
    }
    for (int64_t q = 0; q < M; q++) CHECK(out[(size_t)q] == 1 && out[Mz + (size_t)q] == 1);
    for (size_t x = 0; x < (size_t)M * p; x++) CHECK(h2read[x] == 1);
    return (int)T.chunks.size();
}
}  // namespace

int main() {
    store_walk();
    int ran = 0;
    const std::vector<std::vector<int>> calls = {{3}, {3, 17, 63, 64, 65, 130, 200}, {130, 65}, {64, 130, 3, 200, 65}, {320, 257, 64, 64, 700}};
    const std::vector<int> pts = {0, 1, 63, 64, 65, 130};
    for (size_t ci = 0; ci < calls.size(); ci++) {
        std::vector<int> m;
        for (size_t b = 0; b < calls[ci].size(); b++) m.push_back(pts[(b + ci) % pts.size()]);
        for (int p : {1, 2, 16, 17, 33, 64})
            for (size_t post : {(size_t)1, (size_t)600 << 10, (size_t)2 << 30}) { run_call(calls[ci], m, p, post); ran++; }
    }
    CHECK(basis_g_kend(0) == 64 && basis_g_kend(2) == 192 && basis_g_wave_klast(1, 3) == 127 && BASIS_LDS_STRIDE % 32 == 16 && BASIS_LDS_STRIDE >= 64);
    CHECK(BASIS_MAX_P == 64 && 64 % BASIS_KC == 0);
    std::printf("basis_tables ok (%d calls walked)\n", ran);
    return 0;
}
