// hess_tables_test.cpp -- CPU test of hess_tables.h: the sizes and class offsets of medgp_hess_vec's own buffers (the two-plane slab of
// the raw moments, the block sums of the W pass, [beta | diag(W)]), walked by every workgroup of the new launches -- k_hess_moments'
// second pass (k_wgrad's 1-D grid and slab addressing, restated), k_hess_slabsum, k_hess_beta -- and the capacity rule.  Stand-alone
// (own main, no HIP): built with the host compiler and -fsanitize=address,undefined by tests/test_hess.py, so an index mistake shows
// here and not as an out-of-bounds access on a GPU.  The buffers are real allocations of the computed sizes, written at every
// address the kernels write: the sanitizer checks the bounds, the counts that every piece is written exactly once.
// Build and run: make hess_tables_test && ./hess_tables_test
#include "call_plan.h"
#include "hess_tables.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

// a patient's per-output tables as medgp_set_patient builds them: n observations dealt over D outputs (some empty), grouped by output
struct Pat { std::vector<int> seg, roff, coff, meta; };
Pat make_patient(int n, int D, unsigned seed) {
    Pat p;
    std::vector<int> cnt(D, 0);
    for (int i = 0; i < n; i++) { seed = seed * 1664525u + 1013904223u; cnt[(seed >> 16) % (unsigned)D]++; }
    if (D > 2) { cnt[0] += cnt[1]; cnt[1] = 0; }   // an output without observations
    p.seg.assign(D + 1, 0); p.roff.assign(D + 1, 0); p.coff.assign(D + 1, 0);
    for (int d = 0; d < D; d++) {
        const int a = p.seg[d], z = a + cnt[d];
        p.seg[d + 1] = z;
        p.roff[d + 1] = p.roff[d] + (z > a ? (z - 1) / 16 - a / 16 + 1 : 0);
        p.coff[d + 1] = p.coff[d] + (z > a ? (z - 1) / 64 - a / 64 + 1 : 0);
        for (int i = a; i < z; i++) p.meta.push_back(d);
    }
    CHECK((int)p.meta.size() == n);
    return p;
}

// kernels_wgrad.h: workgroup id -> (entry, tile index) of the 1-D tile grid (not serpentine), and the tile index -> (I, J)
bool tile_of(int x, int nbatch, int ntiles, int nbp, int &b, int &tix) {
    if (nbatch >= 64) {
        const int xcd = x & 7, rest = x >> 3;
        b = (rest / ntiles) * 8 + xcd;
        tix = rest % ntiles;
    } else {
        if (x >= nbp * ntiles) return false;
        b = x % nbp;
        tix = x / nbp;
    }
    return b < nbatch;
}

int run_call(const std::vector<int> &en, int Q, int D, int H, int nvec, size_t budget) {
    const int nbatch = (int)en.size();
    PlanRules r;
    r.Q = Q; r.D = D; r.max_batch = nbatch; r.mem_budget = budget;
    BatchPlan P;
    layout_plan(r, en.data(), nbatch, true, P);
    if (P.nwaves > 1 || !hess_fits(P.need_mat, budget)) return 0;
    CHECK((size_t)HESS_MATS * P.need_mat * sizeof(double) <= budget);
    const HessBuffers hb = hess_buffers(P.need_mat, P.need_vec, P.need_slab, nbatch, nvec, H, Q, D);
    const size_t QDD = (size_t)Q * D * D;
    CHECK(hb.mat_doubles == P.need_mat && hb.dir_doubles == (size_t)nbatch * nvec * H);
    CHECK(P.need_slab % 3 == 0 && hb.hislab_doubles == P.need_slab / 3 * 2);
    CHECK(hb.sums_doubles == 5 * nbatch * QDD && hb.vec_doubles == 2 * P.need_vec);
    std::vector<char> hislab(hb.hislab_doubles, 0), sums(hb.sums_doubles, 0), vecs(hb.vec_doubles, 0);
    for (const SizeClass &k : P.cls) {
        const SlabGeom sg = slab_geom(k.ld, Q, D);
        const size_t hstride = hess_hislab_stride(Q, sg.R, sg.C);
        CHECK(k.off_slab % 3 == 0 && hstride * 3 == sg.stride * 2);
        const size_t hi0 = hess_hislab_of(k.off_slab);
        CHECK(hi0 + (size_t)k.count * hstride <= hb.hislab_doubles);
        CHECK(k.off_vec + (size_t)k.count * k.ld <= P.need_vec);
        const int nt64 = k.nbmax;
        const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, k.count, nt64);
        std::vector<Pat> pats;
        for (int b = 0; b < k.count; b++) pats.push_back(make_patient(P.en[(size_t)k.b0 + b], D, 17u * (unsigned)(k.b0 + b) + 3u));
        // k_hess_moments, second pass: every workgroup, every wave, every (row output run) x (column segment) of its tile
        std::vector<int> tiles_seen((size_t)k.count * wg.wg_tiles, 0);
        for (int x = 0; x < wg.grid; x++) {
            int b, tix;
            if (!tile_of(x, k.count, wg.wg_tiles, wg.nbp, b, tix)) continue;
            CHECK(tix >= 0 && tix < wg.wg_tiles);
            tiles_seen[(size_t)b * wg.wg_tiles + tix]++;
            int I = 0;
            while ((I + 1) * (I + 2) / 2 <= tix) I++;
            const int J = tix - I * (I + 1) / 2;
            const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64;
            if (I >= npad / 64) continue;
            const Pat &p = pats[b];
            char *hi = hislab.data() + hi0 + (size_t)b * hstride;
            for (int w = 0; w < 4; w++) {
                const int rg = 4 * I + w;
                int mcur = -2;
                for (int rr = 0; rr <= 16; rr++) {
                    const int i = 64 * I + 16 * w + rr;
                    const int mi = (rr < 16 && i < n) ? p.meta[i] : -1;
                    if (mi == mcur) continue;
                    if (mcur >= 0) {
                        const int rslot = p.roff[mcur] + (rg - p.seg[mcur] / 16);
                        CHECK(rslot >= p.roff[mcur] && rslot < p.roff[mcur + 1] && rslot < sg.R);
                        for (int lane = 0; lane < 64; lane++) {   // the last lane of every column segment stores
                            const int j = 64 * J + lane;
                            if (j >= n) continue;
                            const int mj = p.meta[j];
                            if (lane != 63 && j + 1 < n && p.meta[j + 1] == mj) continue;
                            const int cslot = p.coff[mj] + (J - p.seg[mj] / 64);
                            CHECK(cslot >= p.coff[mj] && cslot < p.coff[mj + 1] && cslot < sg.C);
                            for (int pl = 0; pl < HESS_HI_PLANES; pl++)
                                for (int q = 0; q < Q; q++) hi[((size_t)(pl * Q + q) * sg.R + rslot) * sg.C + cslot]++;
                        }
                    }
                    mcur = mi;
                }
            }
        }
        for (int v : tiles_seen) CHECK(v == 1);
        // k_hess_slabsum: every piece it reads was written exactly once; one sum per (plane, q, d >= e) into [M3 | M4] of the class
        for (int b = 0; b < k.count; b++) {
            const Pat &p = pats[b];
            const char *hi = hislab.data() + hi0 + (size_t)b * hstride;
            const int nbins = D * (D + 1) / 2;
            CHECK(hess_slabsum_grid(Q, D) * 256 >= HESS_HI_PLANES * Q * nbins && (hess_slabsum_grid(Q, D) - 1) * 256 < HESS_HI_PLANES * Q * nbins);
            for (int idx = 0; idx < HESS_HI_PLANES * Q * nbins; idx++) {
                const int pq = idx / nbins, bin = idx - pq * nbins;
                int d = 0;
                while ((d + 1) * (d + 2) / 2 <= bin) d++;
                const int e = bin - d * (d + 1) / 2;
                for (int rs = p.roff[d]; rs < p.roff[d + 1]; rs++) {
                    const int It = (p.seg[d] / 16 + (rs - p.roff[d])) / 4;
                    for (int cs = p.coff[e]; cs < p.coff[e + 1]; cs++) {
                        const int Jt = p.seg[e] / 64 + (cs - p.coff[e]);
                        if (Jt <= It) CHECK(hi[((size_t)pq * sg.R + rs) * sg.C + cs] == 1);
                    }
                }
                const int pl = pq / Q, q = pq - pl * Q;
                sums[((size_t)(3 + pl) * nbatch + k.b0 + b) * QDD + (size_t)q * D * D + d * D + e]++;
            }
            // ... and k_slabsum's three planes on the W view: S, SM, SV of the class
            for (int pl = 0; pl < 3; pl++)
                for (int q = 0; q < Q; q++)
                    for (int d = 0; d < D; d++)
                        for (int e = 0; e <= d; e++) sums[((size_t)pl * nbatch + k.b0 + b) * QDD + (size_t)q * D * D + d * D + e]++;
            // k_hess_beta: 16-row blocks x 4 waves x 4 rows -> beta; the W pass's diagonal tiles -> diag(W) behind it
            const int n = P.en[(size_t)k.b0 + b], npad = (n + 63) / 64 * 64;
            CHECK(hess_beta_grid(nt64) * 16 == k.ld);
            for (int rb = 0; rb < hess_beta_grid(nt64); rb++) {
                if (16 * rb >= npad) continue;
                for (int w = 0; w < 4; w++)
                    for (int l = 0; l < 4; l++) vecs[k.off_vec + (size_t)b * k.ld + 16 * rb + 4 * w + l]++;
            }
            for (int i = 0; i < n; i++) vecs[P.need_vec + k.off_vec + (size_t)b * k.ld + i]++;
            for (int i = 0; i < k.ld; i++) {
                CHECK(vecs[k.off_vec + (size_t)b * k.ld + i] == (i < npad ? 1 : 0));
                CHECK(vecs[P.need_vec + k.off_vec + (size_t)b * k.ld + i] == (i < n ? 1 : 0));
            }
        }
    }
    // the lower triangles of all five planes of every entry were written once, nothing else
    for (size_t pl = 0; pl < HESS_SUMS; pl++)
        for (size_t b = 0; b < (size_t)nbatch; b++)
            for (int q = 0; q < Q; q++)
                for (int d = 0; d < D; d++)
                    for (int e = 0; e < D; e++) CHECK(sums[(pl * nbatch + b) * QDD + (size_t)q * D * D + d * D + e] == (e <= d ? 1 : 0));
    for (char v : hislab) CHECK(v == 0 || v == 1);
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
    {   // a launch of at least 64 entries (the XCD-major id map), Q = 9, D = 5
        std::vector<int> en(70, 65);
        en[3] = 130;
        ran += run_call(en, 9, 5, 200, 1, (size_t)1 << 30);
    }
    CHECK(ran >= 7 && refused >= 6);
    CHECK(hess_fits(4096, (size_t)HESS_MATS * 4096 * 8) && !hess_fits(4097, (size_t)HESS_MATS * 4096 * 8) && hess_fits(0, 0));
    CHECK(hess_hislab_stride(5, 7, 3) == 2 * 5 * 7 * 3 && hess_hislab_of(3 * 5 * 7 * 3) == hess_hislab_stride(5, 7, 3));
    std::printf("hess_tables ok (%d calls walked, %d refused)\n", ran, refused);
    return 0;
}
