// pjvp_tables_test.cpp -- CPU test of pjvp_tables.h: the tile table and the launch chunks of medgp_posterior_jvp_batch, the sizes and
// class offsets of the call's own buffers (Kdot, u, [dmean | dvar]) and the work rows, walked at every address the new kernels
// write -- k_pjvp_solve's two panels per tile and its per-point outputs, k_pjvp_u, k_pjvp_dir's outputs -- and the capacity rule.
// Stand-alone (own main, no HIP): built with the host compiler and -fsanitize=address,undefined by tests/test_posterior_jvp.py, so an
// index mistake shows here and not as an out-of-bounds access on a GPU.  The buffers are real allocations of the computed sizes: the
// sanitizer checks the bounds, the counts that every piece is written exactly as often as the launches say.
// Build and run: make pjvp_tables_test && ./pjvp_tables_test
#include "call_plan.h"
#include "pjvp_tables.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

// en: observations per caller entry, mpts: test points per caller entry.  Returns the number of chunks (0: refused by the capacity rule).
int run_call(const std::vector<int> &en_caller, const std::vector<int> &mpts, int Q, int D, int H, int nvec, size_t mem_budget, size_t post_budget) {
    const int nbatch = (int)en_caller.size();
    PlanRules r;
    r.Q = Q; r.D = D; r.max_batch = nbatch; r.mem_budget = mem_budget;
    BatchPlan P;
    layout_plan(r, en_caller.data(), nbatch, true, P);
    if (P.nwaves > 1 || !pjvp_fits(P.need_mat, mem_budget)) return 0;
    CHECK((size_t)PJVP_MATS * P.need_mat * sizeof(double) <= mem_budget);
    std::vector<int64_t> offsets(nbatch + 1, 0);
    for (int b = 0; b < nbatch; b++) offsets[b + 1] = offsets[b] + mpts[b];
    const int64_t M = offsets[nbatch];
    const PjvpBuffers pb = pjvp_buffers(P.need_mat, P.need_vec, nbatch, nvec, H, Q, D, M);
    CHECK(pb.mat_doubles == P.need_mat && pb.u_doubles == P.need_vec && pb.dir_doubles == (size_t)nbatch * nvec * H);
    CHECK(pb.coef_doubles == (size_t)nbatch * fisher_coef_stride(Q, D));
    CHECK(pb.out_doubles == 2 * pjvp_dvar_offset(M, nvec) && pjvp_dvar_offset(M, nvec) >= (size_t)M * nvec && pb.out_doubles >= 2);
    std::vector<TableClass> cls;
    for (const SizeClass &k : P.cls) cls.push_back({k.b0, k.count, k.ld});
    PointTables<PostTile> T;
    build_pjvp_tiles(cls, P.order.data(), offsets.data(), post_budget, T);
    std::vector<char> work(T.work_need / sizeof(double), 0), kdot(pb.mat_doubles, 0), u(pb.u_doubles, 0), out(pb.out_doubles, 0);
    std::vector<int> pmean((size_t)M, 0);
    std::vector<int> tile_seen(T.tiles.size(), 0);
    int last_cls = -1;
    size_t next_tile = 0;
    for (const TileChunk &ch : T.chunks) {
        CHECK(ch.cls >= last_cls && ch.cls < (int)P.cls.size());   // the chunks of a class are consecutive, classes in order
        last_cls = ch.cls;
        CHECK((size_t)ch.t0 == next_tile && ch.nt >= 1);          // the chunks partition the tile table
        next_tile += (size_t)ch.nt;
        const SizeClass &k = P.cls[ch.cls];
        CHECK(ch.stride == pjvp_work_stride(k.ld) && ch.stride == (size_t)2 * k.ld * 64);
        CHECK((size_t)ch.nt * ch.stride * sizeof(double) <= T.work_need);
        CHECK(ch.nt == 1 || (size_t)ch.nt * ch.stride * sizeof(double) <= post_budget);
        std::fill(work.begin(), work.end(), 0);
        for (int x = 0; x < ch.nt; x++) {   // k_pjvp_solve: blockIdx.x = x
            const PostTile &t = T.tiles[(size_t)ch.t0 + x];
            tile_seen[(size_t)ch.t0 + x]++;
            CHECK(t.e >= 0 && t.e < k.count && t.cnt >= 1 && t.cnt <= POST_TW);
            const int caller = P.order[(size_t)k.b0 + t.e];
            CHECK(t.p0 >= offsets[caller] && (int64_t)t.p0 + t.cnt <= offsets[caller + 1]);
            const int n = P.en[(size_t)k.b0 + t.e], npad = (n + 63) / 64 * 64;
            CHECK(npad <= k.ld);
            char *Wk = work.data() + (size_t)x * ch.stride, *Vf = Wk + (size_t)k.ld * 64;
            for (int c0 = 0; c0 < npad; c0 += 64)
                for (int row = 0; row < 64; row++)
                    for (int col = 0; col < 64; col++) { Wk[(size_t)(c0 + row) * 64 + col]++; Vf[(size_t)(c0 + row) * 64 + col]++; }
            for (int p = t.p0; p < t.p0 + t.cnt; p++) {
                pmean[(size_t)p]++;
                for (int j = 0; j < nvec; j++) { out[(size_t)p * nvec + j]++; out[pjvp_dvar_offset(M, nvec) + (size_t)p * nvec + j]++; }   // k_pjvp_dir, direction j
            }
        }
        for (char v : work) CHECK(v == 0 || v == 1);   // no two tiles of a chunk share a work row
        // the direction's Kdot (k_fisher_kdot: lower tiles and their mirror images) and u (k_pjvp_u) of the class
        std::fill(kdot.begin(), kdot.end(), 0);
        std::fill(u.begin(), u.end(), 0);
        CHECK(k.off_mat + (size_t)k.count * k.ld * k.ld <= pb.mat_doubles && k.off_vec + (size_t)k.count * k.ld <= pb.u_doubles);
        for (int b = 0; b < k.count; b++) {
            const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64, nb = npad / 64;
            char *Kd = kdot.data() + k.off_mat + (size_t)b * k.ld * k.ld;
            for (int x = 0; x < fisher_kdot_grid(k.nbmax); x++) {
                int I, J;
                fisher_lower_tile(x, I, J);
                if (I >= nb) continue;
                for (int rr = 0; rr < 64; rr++)
                    for (int cc = 0; cc < 64; cc++) {
                        Kd[(size_t)(64 * I + rr) * k.ld + 64 * J + cc]++;
                        if (I != J) Kd[(size_t)(64 * J + rr) * k.ld + 64 * I + cc]++;
                    }
            }
            CHECK(pjvp_u_grid(k.nbmax) * 64 == k.ld);
            for (int x = 0; x < pjvp_u_grid(k.nbmax); x++) {   // k_pjvp_u: blockIdx.x = x, one thread per row of the block
                if (64 * x >= npad) continue;
                for (int lane = 0; lane < 64; lane++) u[k.off_vec + (size_t)b * k.ld + 64 * x + lane]++;
            }
            for (int i = 0; i < k.ld; i++) CHECK(u[k.off_vec + (size_t)b * k.ld + i] == (i < npad ? 1 : 0));
            // what pjvp_mm<2> and k_pjvp_u read of Kdot was written: all of [0, npad)^2
            for (int i = 0; i < npad; i++)
                for (int j = 0; j < npad; j++) CHECK(Kd[(size_t)i * k.ld + j] == 1);
        }
    }
    CHECK(next_tile == T.tiles.size());
    for (int v : tile_seen) CHECK(v == 1);
    for (int64_t p = 0; p < M; p++) {   // every point belongs to exactly one tile; every (point, direction) output is written once
        CHECK(pmean[(size_t)p] == 1);
        for (int j = 0; j < nvec; j++) CHECK(out[(size_t)p * nvec + j] == 1 && out[pjvp_dvar_offset(M, nvec) + (size_t)p * nvec + j] == 1);
    }
    return (int)T.chunks.size() + 1;
}
}  // namespace

int main() {
    int ran = 0, refused = 0, cut = 0;
    const std::vector<std::vector<int>> calls = {{1}, {3, 63, 64, 65}, {130, 200, 1, 64, 65, 512}, {200, 130}, {320, 257, 64, 64, 700}};
    const std::vector<int> pts = {0, 1, 63, 64, 65, 130};
    for (size_t ci = 0; ci < calls.size(); ci++) {
        std::vector<int> m;
        for (size_t b = 0; b < calls[ci].size(); b++) m.push_back(pts[(b + ci) % pts.size()]);
        for (size_t mem : {(size_t)64 << 10, (size_t)1 << 20, (size_t)3 << 20, (size_t)64 << 20})
            for (size_t post : {(size_t)1, (size_t)300 << 10, (size_t)2 << 30}) {
                const int r = run_call(calls[ci], m, 2, 3, 25, 2, mem, post);
                ran += r > 0; refused += !r;
                int ntiles = 0;
                for (int x : m) ntiles += (x + 63) / 64;
                if (r > 0 && post == 1) CHECK(r - 1 == ntiles);   // a budget below one tile: one tile per chunk
                if (r > 0 && r - 1 > (int)calls[ci].size()) cut++;
            }
    }
    {   // no points at all; Q = 9, D = 5, three directions
        CHECK(run_call({65, 130}, {0, 0}, 9, 5, 200, 3, (size_t)1 << 30, (size_t)2 << 30) == 1);
        ran++;
    }
    CHECK(ran >= 7 && refused >= 6 && cut >= 3);
    CHECK(pjvp_fits(4096, (size_t)PJVP_MATS * 4096 * 8) && !pjvp_fits(4097, (size_t)PJVP_MATS * 4096 * 8) && pjvp_fits(0, 0));
    CHECK(pjvp_work_stride(192) == (size_t)2 * 192 * 64 && pjvp_dvar_offset(0, 3) == 3 && pjvp_dvar_offset(5, 3) == 15);
    std::printf("pjvp_tables ok (%d calls walked, %d refused, %d cut into several launches)\n", ran, refused, cut);
    return 0;
}
