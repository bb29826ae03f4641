// mean_tables_test.cpp -- CPU test of mean_tables.h: the element maps, the sizes of the call's own buffers, the grids and the capacity
// rule of medgp_mean_nlml_grad / medgp_mean_posterior_batch, walked at every address k_mean_g, k_mean_panel and k_mean_post touch
// through them (the loops below restate the kernels' index ranges over the same maps).  Stand-alone (own main, no HIP): built with the
// host compiler and -fsanitize=address,undefined by tests/test_mean_truth.py, so an index mistake shows here and not as an
// out-of-bounds access on a GPU.  The buffers are real allocations of the computed sizes: the sanitizer checks the bounds, the counts
// that every element of G, PH, Pm and alpha~ of an entry's own blocks is written exactly once and that everything read was written.
// Build and run: make mean_tables_test && ./mean_tables_test
#include "call_plan.h"
#include "mean_tables.h"
#include "pjvp_tables.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

constexpr int WG_KC = 32;   // the chunk of the tile product (kernels_wgrad.h)

// en: observations per caller entry, mpts: test points per caller entry.  Returns 1 + launch chunks of the posterior; 0: refused.
int run_call(const std::vector<int> &en_caller, const std::vector<int> &mpts, int Q, int D, size_t mem_budget, size_t post_budget) {
    const int nbatch = (int)en_caller.size();
    PlanRules r;
    r.Q = Q; r.D = D; r.max_batch = nbatch; r.mem_budget = mem_budget;
    BatchPlan P;
    layout_plan(r, en_caller.data(), nbatch, true, P);
    if (P.nwaves > 1 || !mean_fits(P.need_mat, P.need_vec, mem_budget)) return 0;
    const MeanBuffers mb = mean_buffers(P.need_vec, nbatch, D);
    CHECK(mb.panel_doubles == 64 * P.need_vec && mb.vec_doubles == 2 * P.need_vec && mb.in_doubles == 2 * (size_t)nbatch * D);
    CHECK(mb.small_doubles == (size_t)nbatch * mean_small_stride(D) && mean_off_cov(D) + (size_t)D * D == mean_small_stride(D));
    CHECK(mean_off_dmean(D) == (size_t)D && mean_off_delta(D) == 2 * (size_t)D && mean_off_ti(D) + (size_t)D * D == mean_off_cov(D));
    CHECK(mean_lam_offset(nbatch, D) + (size_t)nbatch * D == mb.in_doubles && mean_alpha_offset(P.need_vec) + P.need_vec == mb.vec_doubles);
    std::vector<char> G(mb.panel_doubles, 0), PH(mb.panel_doubles, 0), Pm(mb.panel_doubles, 0), vec(mb.vec_doubles, 0), small(mb.small_doubles, 0);
    std::vector<char> U(P.need_mat, 0);   // (read marks only: the sanitizer checks the bounds of the U rows the panel product reads)
    const int k1 = mean_wgrad_k1(D, WG_KC);
    CHECK(k1 >= D && k1 <= MEAN_PW && k1 % WG_KC == 0 && k1 - D < WG_KC);
    for (const SizeClass &k : P.cls) {
        char *Gk = G.data() + MEAN_PW * k.off_vec, *PHk = PH.data() + MEAN_PW * k.off_vec, *Pmk = Pm.data() + MEAN_PW * k.off_vec;
        char *wk = vec.data() + k.off_vec, *ak = vec.data() + mean_alpha_offset(P.need_vec) + k.off_vec, *Uk = U.data() + k.off_mat;
        const int ld = k.ld;
        CHECK(MEAN_PW * (k.off_vec + (size_t)k.count * ld) <= mb.panel_doubles);
        // k_mean_g: grid (mean_g_grid(nbmax), count), lane = row, wave w the columns w (mod 4)
        for (int b = 0; b < k.count; b++)
            for (int blk = 0; blk < mean_g_grid(k.nbmax); blk++) {
                const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64;
                if (64 * blk >= npad) continue;
                for (int lane = 0; lane < 64; lane++)
                    for (int w = 0; w < 4; w++)
                        for (int d = w; d < MEAN_PW; d += 4) {
                            const int i = 64 * blk + lane;
                            if (d < D && i < n)
                                for (int j = 0; j <= i; j += 7) Uk[(size_t)b * ld * ld + (size_t)j * ld + i] = 1;   // U[j][i], j <= i
                            Gk[mean_panel_at(b, ld, i, d)]++;
                        }
            }
        // k_mean_small: one workgroup per entry: w rows < npad, the entry's small block (indexed by the internal entry)
        for (int b = 0; b < k.count; b++) {
            const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64;
            for (int i = 0; i < npad; i++) {
                for (int d = 0; d < D; d++) CHECK(Gk[mean_panel_at(b, ld, i, d)] == 1);
                wk[mean_vec_at(b, ld, i)]++;
            }
            char *sm = small.data() + ((size_t)k.b0 + b) * mean_small_stride(D);
            for (int d = 0; d < D; d++) { sm[mean_off_beta(D) + d]++; sm[mean_off_dmean(D) + d]++; sm[mean_off_delta(D) + d]++; }
            for (int x = 0; x < D * D; x++) { sm[mean_off_ti(D) + x]++; sm[mean_off_cov(D) + x]++; }
        }
        // k_mean_panel: grid (mean_panel_grid(nbmax), count): block I reads G rows [64 I, npad) and U[row][k], k in that range; writes
        // its 64 rows of PH, Pm (all 64 columns) and alpha~
        for (int b = 0; b < k.count; b++)
            for (int I = 0; I < mean_panel_grid(k.nbmax); I++) {
                const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64;
                if (64 * I >= npad) continue;
                const int nct = (D + 15) / 16;
                for (int kk = mean_panel_k0(I); kk < npad; kk++) {
                    for (int ct = 0; ct < nct; ct++)
                        for (int li = 0; li < 16; li++) CHECK(Gk[mean_panel_at(b, ld, kk, 16 * ct + li)] == 1);
                    for (int rl = 0; rl < 64; rl++)
                        if (64 * I + rl < n && kk < n && kk >= 64 * I + rl) Uk[(size_t)b * ld * ld + (size_t)(64 * I + rl) * ld + kk] = 1;
                }
                for (int rl = 0; rl < 64; rl++) {
                    for (int col = 0; col < MEAN_PW; col++) { PHk[mean_panel_at(b, ld, 64 * I + rl, col)]++; Pmk[mean_panel_at(b, ld, 64 * I + rl, col)]++; }
                    ak[mean_vec_at(b, ld, 64 * I + rl)]++;
                }
            }
        // k_mean_wgrad: tile (I, J) reads the Pm rows of both blocks, columns [0, k1), and alpha~ of both blocks
        for (int b = 0; b < k.count; b++) {
            const int n = P.en[(size_t)k.b0 + b], nb64 = (n + 63) / 64;
            for (int I = 0; I < nb64; I++)
                for (int row = 64 * I; row < 64 * I + 64; row++) {
                    for (int col = 0; col < k1; col++) CHECK(Pmk[mean_panel_at(b, ld, row, col)] == 1);
                    CHECK(ak[mean_vec_at(b, ld, row)] == 1);
                }
        }
    }
    // written exactly once inside every entry's own blocks, never outside them
    for (const SizeClass &k : P.cls)
        for (int b = 0; b < k.count; b++) {
            const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64;
            for (int i = 0; i < k.ld; i++) {
                const char want = i < npad ? 1 : 0;
                for (int col = 0; col < MEAN_PW; col++) {
                    const size_t at = MEAN_PW * k.off_vec + mean_panel_at(b, k.ld, i, col);
                    CHECK(G[at] == want && PH[at] == want && Pm[at] == want);
                }
                CHECK(vec[k.off_vec + mean_vec_at(b, k.ld, i)] == want && vec[mean_alpha_offset(P.need_vec) + k.off_vec + mean_vec_at(b, k.ld, i)] == want);
            }
        }
    for (char v : small) CHECK(v == 1);
    // the posterior: pjvp_tables.h's tiles and chunks; k_mean_post reads V (second panel of the tile's work rows) and G, rows < npad
    std::vector<int64_t> offsets(nbatch + 1, 0);
    for (int b = 0; b < nbatch; b++) offsets[b + 1] = offsets[b] + mpts[b];
    const int64_t M = offsets[nbatch];
    std::vector<TableClass> cls;
    for (const SizeClass &k : P.cls) cls.push_back({k.b0, k.count, k.ld});
    PointTables<PostTile> T;
    build_pjvp_tiles(cls, P.order.data(), offsets.data(), post_budget, T);
    std::vector<char> out(2 * (size_t)(M > 0 ? M : 1), 0), work(T.work_need / sizeof(double) + 1, 0);
    for (const TileChunk &ch : T.chunks) {
        const SizeClass &k = P.cls[ch.cls];
        CHECK((size_t)ch.nt * ch.stride * sizeof(double) <= T.work_need && ch.stride == pjvp_work_stride(k.ld));
        std::fill(work.begin(), work.end(), 0);
        for (int x = 0; x < ch.nt; x++)   // k_pjvp_solve: both panels of work row x
            for (size_t i = 0; i < ch.stride; i++) work[(size_t)x * ch.stride + i]++;
        for (int x = 0; x < ch.nt; x++) {
            const PostTile &t = T.tiles[(size_t)ch.t0 + x];
            CHECK(t.e >= 0 && t.e < k.count && t.cnt >= 1 && t.cnt <= POST_TW);
            const int n = P.en[(size_t)k.b0 + t.e], npad = (n + 63) / 64 * 64;
            const char *Vf = work.data() + (size_t)x * ch.stride + (size_t)k.ld * 64;
            for (int kk = 0; kk < npad; kk++) {
                for (int col = 0; col < 64; col++) CHECK(Vf[(size_t)kk * 64 + col] == 1);
                for (int d = 0; d < 16 * ((D + 15) / 16); d++) CHECK(G[MEAN_PW * k.off_vec + mean_panel_at(t.e, k.ld, kk, d)] == 1);
            }
            for (int j = 0; j < t.cnt; j++) { out[(size_t)t.p0 + j]++; out[(size_t)(M > 0 ? M : 1) + t.p0 + j]++; }
        }
    }
    for (int64_t p = 0; p < M; p++) CHECK(out[(size_t)p] == 1 && out[(size_t)M + p] == 1);
    return (int)T.chunks.size() + 1;
}
}  // namespace

int main() {
    int ran = 0, refused = 0, cut = 0;
    const std::vector<std::vector<int>> calls = {{3}, {3, 63, 64, 65, 130}, {130, 65}, {64, 130, 3, 200, 65}, {320, 257, 64, 64, 700}};
    const std::vector<int> pts = {0, 1, 63, 64, 65, 130};
    for (size_t ci = 0; ci < calls.size(); ci++) {
        std::vector<int> m;
        for (size_t b = 0; b < calls[ci].size(); b++) m.push_back(pts[(b + ci) % pts.size()]);
        for (int D : {1, 3, 24, 33, 64})
            for (size_t mem : {(size_t)64 << 10, (size_t)1 << 20, (size_t)64 << 20})
                for (size_t post : {(size_t)1, (size_t)600 << 10, (size_t)2 << 30}) {
                    const int r = run_call(calls[ci], m, 5, D, mem, post);
                    ran += r > 0; refused += r == 0;
                    const int rbig = run_call(calls[ci], m, 5, D, mem, (size_t)2 << 30);
                    CHECK(r <= 0 || (rbig > 0 && r >= rbig));
                    if (r > 0 && r > rbig) cut++;
                }
    }
    CHECK(ran >= 30 && refused >= 10 && cut >= 5);
    // the capacity rule: two matrices and three 64-column panels
    CHECK(mean_fits(4096, 64, (size_t)(2 * 4096 + 3 * 64 * 64) * 8) && !mean_fits(4096, 65, (size_t)(2 * 4096 + 3 * 64 * 64) * 8));
    CHECK(!mean_fits(4097, 0, (size_t)2 * 4096 * 8) && mean_fits(0, 0, 0));
    CHECK(mean_tri_at(0, 0) == 0 && mean_tri_at(63, 63) == 64 * 65 / 2 - 1 && mean_wgrad_k1(1, 32) == 32 && mean_wgrad_k1(33, 32) == 64 && mean_wgrad_k1(64, 32) == 64);
    std::printf("mean_tables ok (%d calls walked, %d refused, %d cut into several launches)\n", ran, refused, cut);
    return 0;
}
