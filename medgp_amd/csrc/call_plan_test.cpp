// call_plan_test.cpp -- CPU test of the plan of a call (call_plan.h) against brute-force restatements: the route rule, the layout of
// size classes, memory waves and arena offsets, the look-ahead scratch layout, the chunks of medgp_screen and the grid of k_wgrad.
// Stand-alone (own main, no HIP): built with the host compiler and -fsanitize=address,undefined by tests/test_call_plan.py, so a wrong
// offset is caught here and not as a workgroup that reads another patient's matrix on a GPU.
// Arguments: the sizes of the heavy-tailed cohort (synth.ragged_sizes(0, 300)); without them that one check is left out.
#include "call_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {
typedef std::mt19937_64 Rng;
int uni(Rng &g, int lo, int hi) { return lo + (int)(g() % (unsigned long long)(hi - lo + 1)); }

PlanRules rules() {
    PlanRules r;
    r.Q = 3; r.D = 4; r.num_cu = 256; r.max_batch = 512;
    r.mem_budget = (size_t)64 << 30;
    return r;
}

// restatements, from the definitions
int nblk(int n) { int nb = 1; while (64 * nb < n) nb++; return nb; }
int bucket(int nb) { for (int j = 0;; j++) if (nb <= (1 << j) && (j == 0 || nb > (1 << (j - 1)))) return j; }
long long cost(int nb) { return (long long)nb * nb * (nb + 17); }

struct Iv { size_t a, b; };   // [a, b)
void check_disjoint_inside(const std::vector<Iv> &v, size_t lo, size_t hi) {
    for (size_t i = 0; i < v.size(); i++) {
        CHECK(v[i].a >= lo && v[i].b <= hi && v[i].a <= v[i].b);
        for (size_t j = 0; j < i; j++) CHECK(v[i].b <= v[j].a || v[j].b <= v[i].a);
    }
}

// ---- uniform calls: the round-4 thresholds -------------------------------------------------------------------------------
int uniform_route(const PlanRules &r, int nb, int count) {
    std::vector<int> en(count, 64 * nb);
    BatchPlan P;
    std::vector<LaNeed> las;
    std::vector<int> la_of;
    layout_plan(r, en.data(), count, true, P);
    CHECK(P.cls.size() == 1 && P.cls[0].count == count && P.cls[0].nbmax == nb);
    choose_routes(r, P, las, la_of);
    CHECK((P.cls[0].route == ROUTE_LA) == (las.size() == 1) && (la_of[0] >= 0) == (las.size() == 1));
    return P.cls[0].route;
}
void test_uniform() {
    const PlanRules r = rules();
    CHECK(uniform_route(r, 2, 8) == 0 && uniform_route(r, 2, 200) == 0);
    CHECK(uniform_route(r, 4, 112) == 2 && uniform_route(r, 4, 113) == 0 && uniform_route(r, 4, 300) == 0);
    CHECK(uniform_route(r, 6, 144) == 2 && uniform_route(r, 6, 145) == 1 && uniform_route(r, 6, 257) == 0);
    for (int nb = 1; nb <= 16; nb++)
        for (int count = 1; count <= 300; count++) {
            int want;
            if (nb >= 3 && count <= (nb <= 4 ? 112 : 144)) want = 2;
            else want = (count > 256 || nb <= 4) ? 0 : 1;
            CHECK(uniform_route(r, nb, count) == want);
        }
}

// ---- the heavy-tailed cohort ----------------------------------------------------------------------------------
void test_cohort(const std::vector<int> &ns) {
    const int want[8][3] = {{1, 92, 2}, {4, 57, 2}, {17, 29, 2}, {53, 16, 2}, {79, 8, 2}, {67, 4, 2}, {58, 2, 0}, {21, 1, 0}};
    const PlanRules r = rules();
    BatchPlan P;
    std::vector<LaNeed> las;
    std::vector<int> la_of;
    layout_plan(r, ns.data(), (int)ns.size(), true, P);
    choose_routes(r, P, las, la_of);
    CHECK(P.cls.size() == 8);
    for (int i = 0; i < 8; i++) CHECK(P.cls[i].count == want[i][0] && P.cls[i].nbmax == want[i][1] && P.cls[i].route == want[i][2]);
}

// ---- layout_plan: brute-force invariants -----------------------------------------------------------------------------------
void check_layout(const PlanRules &r, const std::vector<int> &n, bool with_u, const BatchPlan &P) {
    const int nbatch = (int)n.size();
    CHECK((int)P.order.size() == nbatch && (int)P.inv.size() == nbatch && (int)P.en.size() == nbatch && P.with_u == with_u);
    std::vector<int> seen(nbatch, 0);
    bool ident = true;
    for (int i = 0; i < nbatch; i++) {
        CHECK(P.order[i] >= 0 && P.order[i] < nbatch && !seen[P.order[i]]);
        seen[P.order[i]] = 1;
        CHECK(P.inv[P.order[i]] == i && P.en[i] == n[P.order[i]]);
        ident = ident && P.order[i] == i;
    }
    CHECK(P.identity == ident);
    if (r.no_classes) {   // rounds 1-4: one class in the caller's order, dimensioned by the largest entry
        int mx = 0;
        for (int x : n) mx = std::max(mx, x);
        CHECK(ident && P.cls.size() == 1 && P.nwaves == 1);
        CHECK(P.cls[0].b0 == 0 && P.cls[0].count == nbatch && P.cls[0].nbmax == nblk(mx) && P.cls[0].ld == 64 * nblk(mx));
    }
    for (int i = 0; i + 1 < nbatch && !r.no_classes; i++) {
        CHECK(nblk(P.en[i]) >= nblk(P.en[i + 1]));
        if (nblk(P.en[i]) == nblk(P.en[i + 1])) CHECK(P.order[i] < P.order[i + 1]);   // ties keep the caller's order
    }
    const size_t bpe = with_u ? 16 : 8;
    int next = 0, wave = 0;
    std::vector<Iv> mat, vec, tab, slab;
    size_t end_mat = 0, end_vec = 0, end_tab = 0, end_slab = 0, wave_bytes = 0;
    int wave_entries = 0;   // entries of the open wave
    auto close_wave = [&]() {
        check_disjoint_inside(mat, 0, P.need_mat); check_disjoint_inside(vec, 0, P.need_vec);
        check_disjoint_inside(tab, 0, P.need_tab); check_disjoint_inside(slab, 0, P.need_slab);
        for (const Iv &v : mat) end_mat = std::max(end_mat, v.b);
        for (const Iv &v : vec) end_vec = std::max(end_vec, v.b);
        for (const Iv &v : tab) end_tab = std::max(end_tab, v.b);
        for (const Iv &v : slab) end_slab = std::max(end_slab, v.b);
        // a wave's matrices fit the budget, or the wave is one class of one entry
        if (!r.no_classes) CHECK(wave_bytes <= r.mem_budget || (mat.size() == 1 && wave_entries == 1));
        mat.clear(); vec.clear(); tab.clear(); slab.clear();
        wave_bytes = 0; wave_entries = 0;
    };
    for (size_t ci = 0; ci < P.cls.size(); ci++) {
        const SizeClass &k = P.cls[ci];
        CHECK(k.b0 == next && k.count >= 1 && k.b0 + k.count <= nbatch);   // the classes partition [0, nbatch) in order
        next = k.b0 + k.count;
        int nbmax = 0;
        long long tsum = 0;
        for (int i = k.b0; i < k.b0 + k.count; i++) { nbmax = std::max(nbmax, nblk(P.en[i])); tsum += cost(nblk(P.en[i])); }
        CHECK(k.tsum == tsum);
        if (!r.no_classes) {
            CHECK(k.nbmax == nbmax);
            for (int i = k.b0; i < k.b0 + k.count; i++) CHECK(bucket(nblk(P.en[i])) == bucket(nbmax));
            const size_t per = bpe * (size_t)(64 * nbmax) * (64 * nbmax), cmax = std::max<size_t>(1, r.mem_budget / per);
            CHECK((size_t)k.count <= cmax);
            // a bucket is cut into two classes only by the budget
            if (ci + 1 < P.cls.size() && bucket(P.cls[ci + 1].nbmax) == bucket(nbmax)) CHECK((size_t)k.count == cmax);
        }
        CHECK(k.ld == 64 * k.nbmax);
        CHECK(k.wave == wave || k.wave == wave + 1);   // wave numbers never decrease
        if (k.wave != wave) { close_wave(); wave = k.wave; }
        const size_t ld = k.ld, cnt = k.count, Q = r.Q, D = r.D;
        mat.push_back({k.off_mat, k.off_mat + cnt * ld * ld});
        vec.push_back({k.off_vec, k.off_vec + cnt * ld});
        tab.push_back({k.off_tab, k.off_tab + cnt * Q * ld});
        slab.push_back({k.off_slab, k.off_slab + (with_u ? cnt * 3 * Q * (ld / 16 + D) * (ld / 64 + D) : 0)});
        wave_bytes += bpe * cnt * ld * ld;
        wave_entries += k.count;
    }
    close_wave();
    CHECK(next == nbatch && P.nwaves == wave + 1 && P.cls[0].wave == 0);
    CHECK(P.need_mat == end_mat && P.need_vec == end_vec && P.need_tab == end_tab && P.need_slab == end_slab);
    if (!with_u) CHECK(P.need_slab == 0);
}

std::vector<int> random_sizes(Rng &g, int count) {
    std::vector<int> n(count);
    const int mode = uni(g, 0, 3);
    const int a = uni(g, 1, 6000), b = uni(g, 1, 6000);
    for (int &x : n) {
        if (mode == 0) x = uni(g, 1, 6000);
        else if (mode == 1) x = a;                                // all equal
        else if (mode == 2) x = uni(g, 0, 3) ? a : b;             // two values
        else x = std::min(6000, 1 + (int)(6000.0 / (1 + uni(g, 0, 200))));   // heavy tail, many equal small sizes
    }
    return n;
}

void test_layout() {
    Rng g(20240601);
    BatchPlan P;   // (reused: layout_plan must reset what it finds)
    for (int it = 0; it < 600; it++) {
        PlanRules r = rules();
        r.no_classes = it % 5 == 4;
        r.Q = uni(g, 1, 6); r.D = uni(g, 1, 24);
        const int count = it % 7 == 0 ? 1 : uni(g, 1, 300);
        const std::vector<int> n = random_sizes(g, count);
        const bool with_u = it & 1;
        layout_plan(r, n.data(), count, with_u, P);
        check_layout(r, n, with_u, P);
    }
}

// memory waves: budgets that split the list, one of them smaller than a single entry's matrices
void test_waves() {
    Rng g(77);
    BatchPlan P;
    int split = 0, lone = 0;
    for (int it = 0; it < 400; it++) {
        PlanRules r = rules();
        const int count = uni(g, 1, 300);
        const std::vector<int> n = random_sizes(g, count);
        const bool with_u = it & 1;
        int mx = 0;
        size_t all = 0;
        for (int x : n) { mx = std::max(mx, x); all += (with_u ? 16 : 8) * (size_t)(64 * nblk(x)) * (64 * nblk(x)); }
        const size_t one = (with_u ? 16 : 8) * (size_t)(64 * nblk(mx)) * (64 * nblk(mx));
        const size_t budgets[5] = {one / 2, one, one + one / 2, std::max<size_t>(all / 7, 1), std::max<size_t>(all / 2, 1)};
        r.mem_budget = budgets[it % 5];
        layout_plan(r, n.data(), count, with_u, P);
        check_layout(r, n, with_u, P);
        split += P.nwaves > 1;
        lone += r.mem_budget < one;
    }
    CHECK(split > 100 && lone > 50);
}

// ---- the route of a one-entry call: the expression medgp_get_factor held before it asked choose_routes -----------------------
void test_one_entry() {
    const int mcs[3] = {-1, 0, 1}, nws[3] = {0, 44, 84}, cus[3] = {64, 256, 304};
    for (int nb1 = 1; nb1 <= 130; nb1++)
        for (int mc : mcs) for (int pin = 0; pin <= 1; pin++) for (int nw : nws) for (int v0 = 0; v0 <= 1; v0++) for (int noc = 0; noc <= 1; noc++) for (int cu : cus) {
            PlanRules r = rules();
            r.force_mc = mc; r.pin_route = pin; r.cholinv_nw = nw; r.use_v0 = v0; r.no_classes = noc; r.num_cu = cu;
            const int n = 64 * nb1 - 5;
            const bool la1 = !r.use_v0 && !r.pin_route && nb1 >= 2 && (r.force_mc > 0 || (r.force_mc == 0 && nb1 >= 3));
            const int route1 = la1 ? ROUTE_LA : (r.pin_route ? ROUTE_WG84 : (r.cholinv_nw ? (r.cholinv_nw == 44 ? ROUTE_WG44 : ROUTE_WG84) : (nb1 <= 4 ? ROUTE_WG44 : ROUTE_WG84)));
            BatchPlan P;
            std::vector<LaNeed> las;
            std::vector<int> la_of;
            layout_plan(r, &n, 1, true, P);
            choose_routes(r, P, las, la_of);
            CHECK(P.cls.size() == 1 && P.cls[0].nbmax == nb1 && P.cls[0].route == route1);
            CHECK(las.size() == (la1 ? 1u : 0u) && la_of.size() == 1 && la_of[0] == (la1 ? 0 : -1));
            if (la1) CHECK(las[0].count == 1 && las[0].nbmax == nb1 && las[0].ld == 64 * nb1);
        }
}

// ---- look-ahead scratch: the classes of a wave carved one after another from a lane base ----------------------------------------
void test_la_scratch() {
    Rng g(5);
    for (int it = 0; it < 200; it++) {
        PlanRules r = rules();
        r.force_mc = it % 3 == 0;   // (forced: two-block classes take the schedule as well)
        const std::vector<int> n = random_sizes(g, uni(g, 1, 120));
        const bool with_u = it & 1;
        BatchPlan P;
        std::vector<LaNeed> las;
        std::vector<int> la_of;
        layout_plan(r, n.data(), (int)n.size(), with_u, P);
        P.la_part0 = (size_t)uni(g, 0, 3) * 12345; P.la_small0 = (size_t)uni(g, 0, 3) * 777;
        choose_routes(r, P, las, la_of);
        CHECK(P.nwaves == 1);
        size_t tot_part = 0, tot_small = 0;
        la_needs(P, las, la_of, &tot_part, &tot_small);
        std::vector<Iv> part, small;
        size_t pp = P.la_part0, ps = P.la_small0;   // as ensure_la carves them
        for (const LaNeed &e : las) {
            const LaLayout Y = la_layout(e, with_u);
            // the shapes documented on struct LaArgs
            const size_t cnt = e.count, rows = (with_u ? 2 : 1) * e.nbmax + 1, maxslice = (e.nbmax + 3) / 4, slab = 4096;
            CHECK((size_t)Y.rows == rows && (size_t)Y.maxslice == maxslice);
            for (int k = 0; k < e.nbmax; k++) CHECK((size_t)((k + la_slice_len(k) - 1) / la_slice_len(k)) <= maxslice);   // every slice of every step has a slab
            part.push_back({pp, pp + cnt * 2 * rows * maxslice * slab});
            const size_t offs[8] = {Y.ybuf, Y.xk2, Y.pnx, Y.pnx2, Y.dterm, Y.dsum, Y.dpart, Y.flag};
            const size_t lens[8] = {cnt * 64 * e.ld, cnt * 2 * slab, cnt * 2 * slab, cnt * 2 * slab, cnt * 2 * slab, cnt * 2 * slab, cnt * 2 * maxslice * slab,
                                    (cnt * sizeof(int) + sizeof(double) - 1) / sizeof(double)};
            for (int q = 0; q < 8; q++) small.push_back({ps + offs[q], ps + offs[q] + lens[q]});
            CHECK(part.back().b <= pp + Y.part_doubles && small.back().b <= ps + Y.small_doubles);
            pp += Y.part_doubles; ps += Y.small_doubles;
        }
        check_disjoint_inside(part, P.la_part0, P.la_part0 + tot_part);
        check_disjoint_inside(small, P.la_small0, P.la_small0 + tot_small);
    }
}

// ---- screen_cut ------------------------------------------------------------------------------------------------------------
void test_screen() {
    Rng g(11);
    int twos = 0, works = 0;
    for (int it = 0; it < 300; it++) {
        PlanRules r = rules();
        r.max_batch = uni(g, 1, 3) == 1 ? uni(g, 1, 8) : uni(g, 16, 512);
        r.screen_lanes = 1 + (it & 1);
        r.screen_budget = (size_t)1 << uni(g, 22, 31);
        r.screen_work = (long long)1 << uni(g, 10, 16);
        std::vector<int> walk = random_sizes(g, uni(g, 1, 12));
        std::sort(walk.begin(), walk.end(), [](int a, int b) { return a > b; });
        const int ninit = uni(g, 1, 60);
        const size_t total = walk.size() * (size_t)ninit;
        ScreenCut S;
        screen_cut(r, walk, ninit, S);
        auto nb_of = [&](size_t e) { return nblk(walk[e / ninit]); };
        auto per_of = [&](size_t e) { const size_t ldb = (size_t)64 << bucket(nb_of(e)); return 8 * ldb * ldb; };
        // does one chunk of at most max_batch entries hold everything?
        bool all_in_one = total <= (size_t)r.max_batch;
        {
            size_t bytes = 0; long long work = 0;
            for (size_t e = 0; e < total && all_in_one; e++) {
                if (e > 0 && (bytes + per_of(e) > r.screen_budget || (nb_of(e) >= 45 && work >= r.screen_work))) all_in_one = false;
                bytes += per_of(e); work += (long long)nb_of(e) * nb_of(e);
            }
        }
        CHECK(S.two == (r.screen_lanes >= 2 && r.max_batch >= 2 && !all_in_one));
        CHECK(S.lane_rows == (S.two ? r.max_batch / 2 : r.max_batch));
        twos += S.two;
        size_t next = 0;
        for (const ScreenChunk &ch : S.chunks) {
            CHECK(ch.e0 == next && ch.e1 > ch.e0 && ch.e1 <= total);   // the chunks tile [0, total)
            next = ch.e1;
            CHECK(ch.e1 - ch.e0 <= (size_t)S.lane_rows);
            size_t bytes = 0; long long work = 0;
            for (size_t e = ch.e0; e < ch.e1; e++) {
                if (e > ch.e0 && nb_of(e) >= 45) CHECK(work < r.screen_work);   // closed once its work reaches screen_work
                bytes += per_of(e); work += (long long)nb_of(e) * nb_of(e);
            }
            CHECK(bytes <= r.screen_budget || ch.e1 - ch.e0 == 1);
            if (ch.e1 < total) {   // ... and it was closed for a reason
                const bool by_work = nb_of(ch.e1) >= 45 && work >= r.screen_work;
                CHECK(ch.e1 - ch.e0 == (size_t)S.lane_rows || bytes + per_of(ch.e1) > r.screen_budget || by_work);
                works += by_work;
            }
            // the capacities cover the chunk laid out on its own
            std::vector<int> en;
            for (size_t e = ch.e0; e < ch.e1; e++) en.push_back(walk[e / ninit]);
            BatchPlan P;
            std::vector<LaNeed> las;
            std::vector<int> la_of;
            layout_plan(r, en.data(), (int)en.size(), false, P);
            choose_routes(r, P, las, la_of);
            size_t lp = 0, ls = 0;
            la_needs(P, las, la_of, &lp, &ls);
            CHECK(S.cap_mat >= P.need_mat && S.cap_vec >= P.need_vec && S.cap_tab >= P.need_tab && S.cap_part >= lp && S.cap_small >= ls);
            const PlanNeeds nd = plan_needs(r, P, las, la_of);
            CHECK(nd.mat == P.need_mat && nd.vec == P.need_vec && nd.tab == P.need_tab && nd.slab == P.need_slab && nd.la_part == lp && nd.la_small == ls);
        }
        CHECK(next == total);
    }
    CHECK(twos > 30 && works > 10);
}

// ---- wgrad_grid against its definition ---------------------------------------------------------------------------------------
void test_wgrad_grid() {
    Rng g(3);
    const int counts[9] = {1, 2, 7, 8, 9, 63, 64, 65, 200};
    for (int nbatch : counts)
        for (int rag = 0; rag <= 1; rag++)
            for (int nt64 = 1; nt64 <= 20; nt64 += 3) {
                std::vector<int> n(nbatch, 64 * nt64 - uni(g, 0, 63));
                if (rag && nbatch > 1 && nt64 > 1) n[uni(g, 1, nbatch - 1)] = 64 * (nt64 - 1);
                bool ragged = false;
                for (int x : n) ragged = ragged || nblk(x) != nblk(n[0]);
                CHECK(ragged == (rag && nbatch > 1 && nt64 > 1));
                const int nbp = (ragged && nbatch < 64) ? (nbatch | 1) : nbatch;
                const WgradGrid w = wgrad_grid(n.data(), nbatch, nt64);
                CHECK(w.ragged == ragged && w.nbp == nbp && w.wg_tiles == nt64 * (nt64 + 1) / 2);
                CHECK(w.grid == std::max((nbatch + 7) / 8 * 8, nbp) * w.wg_tiles);
                CHECK(w.nbp >= nbatch && w.grid >= w.nbp * w.wg_tiles);   // every (entry, tile) pair has a workgroup
            }
}

// ---- epilogue_parts against its definition: every (entries, CUs, hypers, room) of the ranges below ------------------------------------
void test_epilogue_parts() {
    for (int nbatch = 1; nbatch <= 300; nbatch++)
        for (int num_cu : {1, 2, 64, 255, 256, 304})
            for (int H = 1; H <= 3000; H += (H < 520 ? 1 : 97))
                for (int max_parts : {1, 2, 8, 16}) {
                    const int ceil256 = H / 256 + (H % 256 ? 1 : 0);
                    const int want = 2 * nbatch >= num_cu ? 1 : (ceil256 < max_parts ? ceil256 : max_parts);
                    const int got = epilogue_parts(nbatch, num_cu, H, max_parts);
                    CHECK(got == want && got >= 1 && got <= max_parts);
                }
}
}  // namespace

// scatter_entry_blocks against the loop it replaced: a non-identity order, a failed entry (NaN rows, also where the device left
// numbers), D = 1 (pieces of one double), a null destination, and exactly-sized destinations (ASan sees a row too many)
void test_scatter() {
    for (int D : {1, 2, 5}) {
        const int nbatch = 4, order[nbatch] = {2, 0, 3, 1}, status[nbatch] = {0, -1, 0, 2};   // (status: the caller's order; 2 = jitter rounds)
        const size_t stride = 3 + (size_t)D + (size_t)D * D, off_a = 1, off_m = 3 + (size_t)D;
        std::vector<double> src(nbatch * stride);
        for (size_t x = 0; x < src.size(); x++) src[x] = 1000.0 + (double)x;
        std::vector<double> a((size_t)nbatch * D, -1.0), m((size_t)nbatch * D * D, -1.0), one(nbatch, -1.0);
        scatter_entry_blocks(order, status, nbatch, src.data(), stride,
                             {{off_a, (size_t)D, a.data()}, {0, 5, nullptr}, {off_m, (size_t)D * D, m.data()}, {0, 1, one.data()}});
        for (int i = 0; i < nbatch; i++) {
            const int b = order[i];
            const bool ok = status[b] >= 0;
            for (int d = 0; d < D; d++) CHECK(ok ? a[(size_t)b * D + d] == src[i * stride + off_a + d] : a[(size_t)b * D + d] != a[(size_t)b * D + d]);
            for (int x = 0; x < D * D; x++) CHECK(ok ? m[(size_t)b * D * D + x] == src[i * stride + off_m + x] : m[(size_t)b * D * D + x] != m[(size_t)b * D * D + x]);
            CHECK(ok ? one[b] == src[i * stride] : one[b] != one[b]);
        }
        CHECK(a[(size_t)1 * D] != a[(size_t)1 * D] && one[0] == src[1 * stride]);   // caller row 1 failed; caller row 0 is internal entry 1
    }
    scatter_entry_blocks(nullptr, nullptr, 0, nullptr, 0, {{0, 1, nullptr}});   // an empty call touches nothing
}

int main(int argc, char **argv) {
    std::vector<int> cohort;
    for (int i = 1; i < argc; i++) cohort.push_back(std::atoi(argv[i]));
    test_uniform();
    if (!cohort.empty()) test_cohort(cohort);
    test_layout();
    test_waves();
    test_one_entry();
    test_la_scratch();
    test_screen();
    test_wgrad_grid();
    test_epilogue_parts();
    test_scatter();
    std::printf("call_plan ok (cohort of %d sizes)\n", (int)cohort.size());
    return 0;
}
