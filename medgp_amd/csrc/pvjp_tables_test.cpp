// pvjp_tables_test.cpp -- CPU test of pvjp_tables.h: the by-covariate order of the points, the tile table, the per-entry records and
// the launch chunks of medgp_posterior_vjp_batch, the sizes of the call's own buffers and the capacity rules, walked at every address the
// new kernels touch through these tables -- the work rows k_pvjp_cot, k_pvjp_wgrad and k_pvjp_cross read (tile0 + j / 64 of the chunk),
// the per-point arrays, c, the per-entry sums and the gradient rows.  Stand-alone (own main, no HIP): built with the host compiler and
// -fsanitize=address,undefined by tests/test_posterior_vjp.py, so an index mistake shows here and not as an out-of-bounds access on a
// GPU.  The buffers are real allocations of the computed sizes: the sanitizer checks the bounds, the counts that every piece is
// touched exactly as often as the launches say.
// Build and run: make pvjp_tables_test && ./pvjp_tables_test
#include "call_plan.h"
#include "pvjp_tables.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

// en: observations per caller entry, mpts: test points per caller entry.  Returns 1 + the number of chunks; 0: refused by the matrix
// rule; -1: refused because one entry's work rows exceed the budget.
int run_call(const std::vector<int> &en_caller, const std::vector<int> &mpts, int Q, int D, int H, int ncot, size_t mem_budget, size_t post_budget,
             bool with_meta) {
    const int nbatch = (int)en_caller.size();
    PlanRules r;
    r.Q = Q; r.D = D; r.max_batch = nbatch; r.mem_budget = mem_budget;
    BatchPlan P;
    layout_plan(r, en_caller.data(), nbatch, true, P);
    if (P.nwaves > 1 || !pvjp_fits(P.need_mat, mem_budget)) return 0;
    std::vector<int64_t> offsets(nbatch + 1, 0);
    for (int b = 0; b < nbatch; b++) offsets[b + 1] = offsets[b] + mpts[b];
    const int64_t M = offsets[nbatch];
    std::vector<int32_t> meta2((size_t)M);
    for (int64_t p = 0; p < M; p++) meta2[(size_t)p] = (int32_t)((p * 7 + 3) % D);   // unsorted; D - 1 may stay empty for short ranges
    std::vector<TableClass> cls;
    for (const SizeClass &k : P.cls) cls.push_back({k.b0, k.count, k.ld});
    PvjpTables T;
    TableError err{};
    if (!build_pvjp_tables(cls, P.order.data(), offsets.data(), with_meta ? meta2.data() : nullptr, nbatch, D, post_budget, T, err)) {
        CHECK(err.b >= 0 && err.b < nbatch && P.order[(size_t)err.entry] == err.b && err.need > post_budget && err.m == mpts[(size_t)err.b]);
        return -1;
    }
    const PvjpBuffers pb = pvjp_buffers(P.need_vec, nbatch, ncot, H, Q, D, M);
    const size_t Mz = pvjp_mz(M);
    CHECK(Mz >= 1 && Mz >= (size_t)M && pb.in_doubles == (2 * (size_t)ncot + 2) * Mz && pb.pts_doubles == (5 + 2 * (size_t)Q) * Mz && pvjp_moments_offset(Q, M) + 2 * Mz == pb.pts_doubles);
    CHECK(pb.vec_doubles >= P.need_vec && pb.small_doubles == (size_t)nbatch * (D + 2) && pb.out_doubles == (size_t)ncot * nbatch * H);
    // the order: a permutation that stays inside every patient's range and is stably sorted by covariate
    CHECK(T.src.size() == (size_t)M && T.dev_of.size() == (size_t)M);
    for (int b = 0; b < nbatch; b++)
        for (int64_t k = offsets[b]; k < offsets[b + 1]; k++) {
            const int64_t s = T.src[(size_t)k];
            CHECK(s >= offsets[b] && s < offsets[b + 1] && T.dev_of[(size_t)s] == (int)k);
            if (k > offsets[b] && with_meta) {
                const int64_t s0 = T.src[(size_t)k - 1];
                CHECK(meta2[(size_t)s0] < meta2[(size_t)s] || (meta2[(size_t)s0] == meta2[(size_t)s] && s0 < s));
            }
            if (!with_meta) CHECK(s == k);
        }
    std::vector<char> work(T.work_need / sizeof(double), 0), pts(pb.pts_doubles, 0), cvec(pb.vec_doubles, 0), small(pb.small_doubles, 0), out(pb.out_doubles, 0);
    std::vector<int> tile_seen(T.tiles.size(), 0), ent_seen((size_t)nbatch, 0);
    int last_cls = -1, next_e = 0;
    size_t next_tile = 0;
    for (const PvjpChunk &ch : T.chunks) {
        CHECK(ch.cls >= last_cls && ch.cls < (int)P.cls.size());   // the chunks of a class are consecutive, classes in order
        if (ch.cls != last_cls) next_e = 0;
        last_cls = ch.cls;
        const SizeClass &k = P.cls[ch.cls];
        CHECK(ch.e0 == next_e && ch.ne >= 1 && ch.e0 + ch.ne <= k.count);   // the chunks partition the class's entries ...
        next_e += ch.ne;
        CHECK((size_t)ch.t0 == next_tile && ch.nt >= 0);                     // ... and the tile table
        next_tile += (size_t)ch.nt;
        CHECK(ch.stride == pjvp_work_stride(k.ld));
        CHECK((size_t)ch.nt * ch.stride * sizeof(double) <= T.work_need && (size_t)ch.nt * ch.stride * sizeof(double) <= post_budget);
        std::fill(work.begin(), work.end(), 0);
        for (int x = 0; x < ch.nt; x++) {   // k_pjvp_solve: blockIdx.x = x writes both panels of work row x
            const PostTile &t = T.tiles[(size_t)ch.t0 + x];
            tile_seen[(size_t)ch.t0 + x]++;
            CHECK(t.e >= ch.e0 && t.e < ch.e0 + ch.ne && t.cnt >= 1 && t.cnt <= POST_TW);   // a tile's entry is in the tile's chunk
            char *Wk = work.data() + (size_t)x * ch.stride;
            for (size_t i = 0; i < ch.stride; i++) Wk[i]++;
        }
        for (int el = 0; el < ch.ne; el++) {   // the entry kernels: blockIdx = el, records ents + k.b0 + ch.e0
            const int i = k.b0 + ch.e0 + el;
            const PvjpEnt &E = T.ents[(size_t)i];
            ent_seen[(size_t)i]++;
            const int caller = P.order[(size_t)i], n = P.en[(size_t)i], npad = (n + 63) / 64 * 64;
            CHECK(E.ent == i && E.p0 == offsets[caller] && E.m == mpts[(size_t)caller] && npad <= k.ld);
            const int nt = (E.m + 63) / 64;
            CHECK(E.tile0 >= 0 && E.tile0 + nt <= ch.nt);
            for (int tt = 0; tt < nt; tt++) {   // the entry's tiles are its own, in point order
                const PostTile &t = T.tiles[(size_t)ch.t0 + E.tile0 + tt];
                CHECK(t.e == ch.e0 + el && t.p0 == E.p0 + 64 * tt && t.cnt == std::min(64, E.m - 64 * tt));
            }
            for (int j = 0; j < E.m; j++)       // every W / V element the kernels read was written by k_pjvp_solve of this chunk
                for (int row = 0; row < npad; row += 17)
                    for (int panel = 0; panel < 2; panel++)
                        CHECK(work[(size_t)(E.tile0 + (j >> 6)) * ch.stride + (size_t)panel * k.ld * 64 + (size_t)row * 64 + (j & 63)] == 1);
            for (int j = 0; j < E.m; j++) {
                for (int a = 0; a < 3; a++) pts[(size_t)a * Mz + E.p0 + j]++;
                for (int q = 0; q < 2 * Q + 2; q++) pts[(3 + (size_t)q) * Mz + E.p0 + j]++;
            }
            CHECK(k.off_vec + (size_t)(ch.e0 + el + 1) * k.ld <= pb.vec_doubles);
            for (int row = 0; row < npad; row++) cvec[k.off_vec + (size_t)(ch.e0 + el) * k.ld + row]++;
            for (int d = 0; d < D + 2; d++) small[(size_t)i * (D + 2) + d]++;
            for (int s = 0; s < ncot; s++)
                for (int h = 0; h < H; h++) out[((size_t)s * nbatch + caller) * H + h]++;
            // the covariate ranges
            const int *ps = T.pseg.data() + (size_t)i * (D + 1);
            CHECK(ps[0] == 0 && ps[D] == E.m);
            for (int d = 0; d < D; d++) {
                CHECK(ps[d] <= ps[d + 1]);
                for (int j = ps[d]; j < ps[d + 1]; j++) CHECK((with_meta ? meta2[(size_t)T.src[(size_t)E.p0 + j]] : 0) == d);
            }
        }
    }
    CHECK(next_tile == T.tiles.size());
    for (int v : tile_seen) CHECK(v == 1);
    for (int v : ent_seen) CHECK(v == 1);   // every entry -- one without points too -- belongs to exactly one chunk
    for (int64_t p = 0; p < M; p++)
        for (int a = 0; a < 5 + 2 * Q; a++) CHECK(pts[(size_t)a * Mz + (size_t)p] == 1);
    for (char v : small) CHECK(v == 1);
    for (char v : out) CHECK(v == 1);
    for (char v : cvec) CHECK(v == 0 || v == 1);
    return (int)T.chunks.size() + 1;
}
}  // namespace

int main() {
    int ran = 0, refused = 0, cut = 0, toolarge = 0;
    const std::vector<std::vector<int>> calls = {{1}, {3, 63, 64, 65}, {130, 200, 1, 64, 65, 512}, {200, 130}, {320, 257, 64, 64, 700}};
    const std::vector<int> pts = {0, 1, 63, 64, 65, 130};
    for (size_t ci = 0; ci < calls.size(); ci++) {
        std::vector<int> m;
        for (size_t b = 0; b < calls[ci].size(); b++) m.push_back(pts[(b + ci) % pts.size()]);
        for (size_t mem : {(size_t)64 << 10, (size_t)1 << 20, (size_t)3 << 20, (size_t)64 << 20})
            for (size_t post : {(size_t)1, (size_t)600 << 10, (size_t)3 << 20, (size_t)2 << 30})
                for (bool with_meta : {true, false}) {
                    const int r = run_call(calls[ci], m, 2, 3, 25, 1 + (int)(ci % 3), mem, post, with_meta);
                    ran += r > 0; refused += r == 0; toolarge += r < 0;
                    const int rbig = run_call(calls[ci], m, 2, 3, 25, 1, mem, (size_t)2 << 30, with_meta);   // one chunk per size class
                    CHECK(r <= 0 || (rbig > 0 && r >= rbig));
                    if (r > 0 && r > rbig) cut++;
                }
    }
    {   // no points at all; Q = 9, D = 5, three cotangent sets: one chunk per class, no tile
        CHECK(run_call({65, 130}, {0, 0}, 9, 5, 200, 3, (size_t)1 << 30, (size_t)2 << 30, true) >= 2);
        ran++;
    }
    CHECK(ran >= 7 && refused >= 6 && cut >= 1 && toolarge >= 3);
    CHECK(pvjp_fits(4096, (size_t)PVJP_MATS * 4096 * 8) && !pvjp_fits(4097, (size_t)PVJP_MATS * 4096 * 8) && pvjp_fits(0, 0));
    CHECK(pvjp_mz(0) == 1 && pvjp_mz(5) == 5 && pvjp_cross_grid(1) == 1 && pvjp_cross_grid(24) == 75 && pvjp_cross_grid(3) == 2);
    std::printf("pvjp_tables ok (%d calls walked, %d refused, %d with an entry above the budget, %d cut into several launches)\n", ran, refused, toolarge, cut);
    return 0;
}
