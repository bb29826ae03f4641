// call_plan.h -- the plan of a call: internal order, size classes, memory waves, arena offsets and needs, factorisation routes, the
// look-ahead scratch layout, the chunks of medgp_screen, the grid of the gradient kernels and the scatter of per-entry result blocks to the caller's rows.
// Plain C++ on plain data (no HIP header, no kernel, no context): medgp_capi.hip includes it for the planning functions,
// kernels_cholinv_la.h for the look-ahead constants, and call_plan_test.cpp compiles it alone with the host compiler, under sanitizers,
// against brute-force restatements.  This arithmetic decides which memory a workgroup touches.
// Inputs: the sizes of the call's entries and the rule inputs of the context (PlanRules).
#pragma once
#include <algorithm>
#include <cstddef>
#include <initializer_list>
#include <limits>
#include <vector>

#ifndef MEDGP_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define MEDGP_HD __host__ __device__
#else
#define MEDGP_HD
#endif
#endif

// ---- look-ahead constants that size the scratch (kernels_cholinv_la.h) -----------------------------------------------------
#define LA_SLICE 4        // panels (64 columns each) per look-ahead slice: the shortest slice (scratch is dimensioned for it)
// Panels per slice of the partial sums PRODUCED at step k (consumed one step later).  It depends on the step alone -- not on the batch
// or on the batch-mates' sizes, so a patient's arithmetic is the same in any call.  Late steps of a long factorisation use longer
// slices: a single N = 4096 evaluation has 526-600 tasks per step from k = 37 on, a few more than the chip's 512 workgroup slots,
// and paid a second, nearly empty round of 24-us tasks per step.  Measured at N = 4096 (k_la_step, interleaved on one box): 4 panels
// throughout 2.20 ms; 5 from step 36 2.17; 5 from 36 + 6 from 52 2.11; 5 from 32 + 6 from 44 (this rule) 2.08; longer slices or
// earlier switches 2.09-2.12.  (N <= 2048 never reaches step 32: unchanged.)
MEDGP_HD inline int la_slice_len(int k) { return k < 32 ? LA_SLICE : (k < 44 ? LA_SLICE + 1 : LA_SLICE + 2); }

// ---- the rule inputs: what the plan reads of a context (medgp_ctx::rules is their one home) ----------------------------------
struct PlanRules {
    int Q = 0, D = 0;
    int num_cu = 256;
    int max_batch = 0;
    size_t mem_budget = (size_t)64 << 30;   // bytes of per-entry matrices one wave of a call may use (MEDGP_MEM_BUDGET_GB)
    size_t screen_budget = (size_t)2 << 30; // the same for one chunk of medgp_screen (MEDGP_SCREEN_BUDGET_GB)
    long long screen_work = 32768;  // block pairs (sum nb^2) at which a medgp_screen chunk of look-ahead entries is closed (MEDGP_SCREEN_WORK)
    int screen_lanes = 2;     // MEDGP_SCREEN_LANES=1: one lane (rounds 1-5)
    int no_classes = 0;       // MEDGP_NO_CLASSES=1: rounds 1-4 behaviour -- one class per call, one route from its largest entry (A-B)
    bool use_v0 = false;      // MEDGP_V0=1: the generic (non-templated) pair kernels of the Q > 8 route for any Q (debug / A-B parity)
    int pin_route = 0;        // medgp_pin_route: every entry is factored by k_cholinv<8,4> whatever the batch (reproducible bits)
    int force_mc = 0;         // MEDGP_MULTI_CU=1 forces / -1 forbids the multi-CU factorisation (0 = auto)
    int cholinv_nw = 0;       // MEDGP_CHOLINV_NW=44|84 forces the workgroup shape <waves, 16-row units per wave> (0 = auto)
};

// ---- the plan of a call (round 5) --------------------------------------------------------------------------------------------
// A call's entries are ordered by size internally and cut into SIZE CLASSES (64-block count in (2^(j-1), 2^j]): every class is a view
// of the batch buffers with its own leading dimension (the class's largest n rounded up to 64), its own launch geometry and its own
// factorisation route, and the classes of one call run beside each other on separate streams.  Why: the reference gives patients
// resources by size (ref: scripts/slurm_della.json:6-62, medgpc/util/run_exp_generator.py:213-260); rounds 1-4 chose ONE route per
// call from the call's largest patient, so one N ~ 6000 patient in a batch of 300 ran on one workgroup and set the time of the call.
enum Route { ROUTE_WG44 = 0, ROUTE_WG84 = 1, ROUTE_LA = 2 };
struct SizeClass {
    int b0 = 0, count = 0;     // internal entries [b0, b0 + count)
    int nbmax = 1;             // 64-blocks of the class's largest entry
    int ld = 64;               // leading dimension of the class view
    int wave = 0;              // memory wave of the call the class runs in (round 6; BatchPlan::nwaves)
    size_t off_mat = 0, off_vec = 0, off_tab = 0, off_slab = 0;   // offsets (doubles) of the class inside Kmat/Linv, z/alpha/wdiag, cs/sn, slab (relative to its wave: waves reuse the arenas)
    long long tsum = 0;        // sum of the cost model over its entries (route rule)
    int route = ROUTE_WG84;    // last route taken (diagnostics: medgp_last_plan)
};
struct BatchPlan {
    bool identity = true;      // internal order == caller order
    std::vector<int> order;    // internal index -> caller index
    std::vector<int> inv;      // caller index -> internal index
    std::vector<int> en;       // n of every entry, internal order
    std::vector<SizeClass> cls;
    size_t need_mat = 0, need_vec = 0, need_tab = 0, need_slab = 0;   // doubles the call needs of each arena (largest wave)
    // Memory waves (round 6): a call whose per-entry matrices exceed the context's budget (512 resident patients of N ~ 6000 would
    // need 296 GB) is run as consecutive WAVES of whole size classes that each fit it; the waves reuse the arenas in stream order.
    int nwaves = 1;
    bool with_u = true;        // laid out for Kmat AND Linv (false: an nlml-only plan, 8 ld^2 bytes per entry instead of 16)
    // Lane base (medgp_screen's two lanes, round 6): the plan's entries use rows [row0, row0 + n) of the batch-indexed buffers and the
    // arenas from these offsets on (doubles), so that two plans can be in flight on two streams at once.  0 for every other call.
    int row0 = 0;
    size_t mat0 = 0, vec0 = 0, tab0 = 0, la_part0 = 0, la_small0 = 0;
};

inline int tri(int n) { return n * (n + 1) / 2; }
inline int blocks64(int n) { return (std::max(n, 1) + 63) / 64; }
// size class of an entry of nb 64-blocks: 0 -> {1}, 1 -> {2}, 2 -> {3, 4}, 3 -> {5 .. 8}, ...
inline int size_bucket(int nb) { int j = 0; while ((1 << j) < nb) j++; return j; }
// Cost model of one entry on ONE workgroup (k_cholinv), fitted to profiles/r04_route_table.txt (ms = 4.4e-4 nb^2 (nb + 17):
// N = 256 0.15, 512 0.70, 768 1.83, 1024 3.7; N = 8192: 1.05 s against 1.33 s measured).  Integer, so the route rule is exact.
inline long long wg_cost(int nb) { return (long long)nb * nb * (nb + 17); }

// The grid of k_wgrad (and of k_loo_kinv / k_loo_wgrad, which walk the same tiles) for a class of nbatch entries of sizes entry_n, nt64
// 64-blocks the largest.  ragged: entries of different 64-block counts in the class.  Entries of different sizes in a launch of few
// entries: odd stride nbp of the entry index, so that every entry's tiles go to all XCDs (kernels_wgrad.h); equally large entries keep
// the stride nbatch (balanced as it is, and the measured form).  grid: workgroups of the launch (its x extent).
struct WgradGrid { bool ragged; int nbp, wg_tiles; int grid; };
inline WgradGrid wgrad_grid(const int *entry_n, int nbatch, int nt64) {
    WgradGrid g{false, nbatch, tri(nt64), 0};
    for (int bb = 1; bb < nbatch; bb++) g.ragged = g.ragged || blocks64(entry_n[bb]) != blocks64(entry_n[0]);
    if (g.ragged && nbatch < 64) g.nbp = nbatch | 1;
    g.grid = std::max(8 * ((nbatch + 7) / 8), g.nbp) * g.wg_tiles;
    return g;
}

// The y extent of the gradient epilogue's grid (k_epilogue, k_hess_epilogue) for a class of nbatch entries of H hypers on num_cu CUs.
// Few entries: the hypers of an entry are spread over workgroups (H = 2954 at D = 64: 0.18 -> 0.07 ms for one entry); with a
// workgroup per CU anyway, one part per entry is faster (each part stages S and A again: 0.09 vs 0.20 ms at 512 entries).
// max_parts: the parts the per-entry partial sums have room for (MEDGP_EPI_PARTS).
inline int epilogue_parts(int nbatch, int num_cu, int H, int max_parts) {
    return (2 * nbatch >= num_cu) ? 1 : std::min(max_parts, (H + 255) / 256);
}

// the gradient slab of one entry of a view of leading dimension ld: 3 Q planes of R x C bins (kernels_wgrad.h); stride in doubles
struct SlabGeom { int R, C; size_t stride; };
inline SlabGeom slab_geom(int ld, int Q, int D) {
    SlabGeom g{ld / 16 + D, ld / 64 + D, 0};
    g.stride = (size_t)3 * Q * g.R * g.C;
    return g;
}

// Lay out the plan of a call from the sizes of its entries alone (en[b] = n of caller entry b): internal order, size classes, memory
// waves, offsets, needs.  with_u: the call forms U = L^-T (gradient / factor outputs / predict); an nlml-only call touches neither
// Linv nor the gradient slab.  Pure host arithmetic: medgp_reserve_plan runs it on announced sizes to find the high-water marks.
inline void layout_plan(const PlanRules &r, const int *en, int nbatch, bool with_u, BatchPlan &P) {
    P.order.resize(nbatch); P.inv.resize(nbatch); P.en.resize(nbatch);
    P.cls.clear();
    P.with_u = with_u;
    int mx = 0;
    for (int b = 0; b < nbatch; b++) { P.order[b] = b; mx = std::max(mx, en[b]); }
    const bool classes = !r.no_classes;
    // by 64-block count, largest first (what the hardware dispatches first runs longest: LPT inside every launch); ties keep the caller's order
    if (classes) std::stable_sort(P.order.begin(), P.order.end(), [&](int a, int b) { return blocks64(en[a]) > blocks64(en[b]); });
    P.identity = true;
    for (int i = 0; i < nbatch; i++) { P.inv[P.order[i]] = i; P.en[i] = en[P.order[i]]; P.identity = P.identity && P.order[i] == i; }
    const size_t Q = r.Q, bpe = with_u ? 16 : 8;   // bytes of per-entry matrices per ld^2
    size_t om = 0, ov = 0, ot = 0, os = 0, wave_bytes = 0;
    int wave = 0;
    P.need_mat = P.need_vec = P.need_tab = P.need_slab = 0;
    for (int i = 0; i < nbatch;) {
        SizeClass k;
        k.b0 = i;
        const int bk = size_bucket(blocks64(P.en[i]));
        k.nbmax = classes ? blocks64(P.en[i]) : blocks64(mx);   // (sorted: the first entry of a class is its largest)
        k.ld = 64 * k.nbmax;
        // a class is cut where its matrices would exceed the budget of one wave (512 entries of N ~ 6000: 296 GB)
        const size_t per = bpe * (size_t)k.ld * k.ld;
        const int cmax = classes ? (int)std::max<size_t>(1, r.mem_budget / per) : nbatch;
        int j = i;
        while (j < nbatch && j - i < cmax && (!classes || size_bucket(blocks64(P.en[j])) == bk)) { k.tsum += wg_cost(blocks64(P.en[j])); j++; }
        k.count = j - i;
        const size_t kbytes = per * k.count;
        if (classes && wave_bytes > 0 && wave_bytes + kbytes > r.mem_budget) { wave++; om = ov = ot = os = 0; wave_bytes = 0; }
        k.wave = wave;
        wave_bytes += kbytes;
        k.off_mat = om; k.off_vec = ov; k.off_tab = ot; k.off_slab = os;
        om += (size_t)k.count * k.ld * k.ld; ov += (size_t)k.count * k.ld; ot += (size_t)k.count * Q * k.ld;
        if (with_u) os += (size_t)k.count * slab_geom(k.ld, r.Q, r.D).stride;
        P.need_mat = std::max(P.need_mat, om); P.need_vec = std::max(P.need_vec, ov); P.need_tab = std::max(P.need_tab, ot); P.need_slab = std::max(P.need_slab, os);
        P.cls.push_back(k);
        i = j;
    }
    P.nwaves = wave + 1;
}

// ---- scratch of the look-ahead factorisation (kernels_cholinv_la.h) --------------------------------------------------------
// A class that takes the look-ahead schedule: count entries, nbmax 64-blocks the largest, ld the leading dimension of its view.
struct LaNeed { int count, nbmax, ld; };
// Where the scratch of one such class lies inside the two look-ahead arenas (doubles): `part` holds the partial-sum slab alone
// ([count][2][rows][maxslice][4096], part_doubles of it); `small` holds the other buffers of struct LaArgs back to back, each at the
// offset named after it from the class's base, small_doubles in all:
//   ybuf [count][64][ld] | xk2, pnx, pnx2, dterm, dsum [count][2][4096] each | dpart [count][2][maxslice][4096] | flag [count] ints
// (one double per entry).  with_u = false (nlml only): no U row blocks, so the partial-sum slab holds nbmax + 1 row blocks, not
// 2 nbmax + 1.  The scratch is dimensioned for the shortest slice (LA_SLICE panels).
struct LaLayout {
    int maxslice, rows;
    size_t ybuf, xk2, pnx, pnx2, dterm, dsum, dpart, flag;
    size_t part_doubles, small_doubles;
};
inline LaLayout la_layout(const LaNeed &e, bool with_u) {
    LaLayout Y{};
    const size_t nb = e.count, hand = nb * 2 * 4096;   // (a hand-off slab of the chain: indexed by parity)
    Y.maxslice = (e.nbmax + LA_SLICE - 1) / LA_SLICE;
    Y.rows = (with_u ? 2 : 1) * e.nbmax + 1;
    Y.part_doubles = nb * 2 * Y.rows * Y.maxslice * 4096;
    Y.ybuf = 0;
    Y.xk2 = Y.ybuf + nb * 64 * e.ld;
    Y.pnx = Y.xk2 + hand;
    Y.pnx2 = Y.pnx + hand;
    Y.dterm = Y.pnx2 + hand;
    Y.dsum = Y.dterm + hand;
    Y.dpart = Y.dsum + hand;
    Y.flag = Y.dpart + nb * 2 * Y.maxslice * 4096;
    Y.small_doubles = Y.flag + nb;
    return Y;
}

// Route rule.  Measured on MI355X, round 4 (scratch/route_sweep.py -> profiles/r04_route_table.txt; factorisation ms per call, nlml +
// gradient, LA = look-ahead schedule, 44 / 84 = k_cholinv<4,4> / <8,4>; the same table at D = 2 and D = 24):
//   N=128: 44 wins at every batch size (0.069 vs LA 0.073 at 8 entries, 0.081 vs 0.112 at 256)
//   N=256: LA <= 96 entries (0.127 / 0.168 vs 44: 0.168 / 0.182 at 8 / 96), 44 from 128 on (0.185 vs LA 0.197)
//   N=384: LA <= 128 (0.390 vs 84: 0.395), 84 from 160 on (0.412 vs LA 0.473)
//   N=512: LA <= 96 (0.560 vs 0.683), tie at 128 (0.709 / 0.705), 84 from 160 on (0.712 vs 0.885)
//   N=768 / 1024: LA <= 128 (1.78 vs 1.86; 3.46 vs 3.69), 84 from 160 on (1.91 vs 2.19; 3.74 vs 4.34)
// The LA time grows linearly with the batch, the single-workgroup time is flat up to one patient per CU.  For a uniform call that gave:
// never for two blocks; up to 7/16 #CU entries (112) for three or four blocks; up to 9/16 #CU (144) from five blocks on.  Round 5 states the
// same rule per size CLASS of a ragged call: with t(nb) the one-workgroup cost model (wg_cost) and S the summed cost of the entries not
// yet given to the look-ahead schedule, a class (largest first) takes the look-ahead schedule when  t(nb_max) * #CU * f >= S  (f = 7/16
// or 9/16 as above) -- i.e. when one of its entries on one workgroup would stick out of the average load per CU of everything that is
// left.  For a uniform call S = n t and the rule is the old one (n <= 112 / 144); in a ragged call the heavy tail is peeled off class by
// class until the rest is balanced.
// routes of the classes of a plan (the rule above); returns the look-ahead scratch entries, la_of[i] = index into them or -1
inline void choose_routes(const PlanRules &r, BatchPlan &P, std::vector<LaNeed> &las, std::vector<int> &la_of) {
    long long S = 0;
    for (const SizeClass &k : P.cls) S += k.tsum;
    las.clear();
    la_of.assign(P.cls.size(), -1);
    for (size_t i = 0; i < P.cls.size(); i++) {
        SizeClass &k = P.cls[i];
        bool la = false;
        if (!r.use_v0 && !r.pin_route && k.nbmax >= 2) {
            if (r.force_mc > 0) la = true;   // (forced, A-B and tests: also for two blocks)
            else if (r.force_mc == 0 && k.nbmax >= 3 && !r.no_classes) la = wg_cost(k.nbmax) * r.num_cu * (k.nbmax <= 4 ? 7 : 9) >= 16 * S;
            else if (r.force_mc == 0 && k.nbmax >= 3) la = k.count <= (r.num_cu * (k.nbmax <= 4 ? 7 : 9)) / 16;   // rounds 1-4: by entry count alone
        }
        if (la) {
            k.route = ROUTE_LA;
            S -= k.tsum;
            la_of[i] = (int)las.size();
            las.push_back({k.count, k.nbmax, k.ld});
        } else {
            // more patients than CUs: 4-wave workgroups, two per CU (the serial diagonal phase of one overlaps the MFMA phase of the
            // other).  At most one patient per CU: 8 waves (8 block slots per pass) once a step has more than 4 row blocks, else the
            // 4-wave shape, whose 4 slots already cover every block of n <= 256 (measured, 256 patients x N=256, D=2: <4,4> 0.211 ms,
            // <8,4> 0.232 ms -- half of its 8 slots idle).
            const int shape = r.pin_route ? 84 : (r.cholinv_nw ? r.cholinv_nw : ((k.count > r.num_cu || k.nbmax <= 4) ? 44 : 84));
            k.route = shape == 44 ? ROUTE_WG44 : ROUTE_WG84;
        }
    }
}

// what a plan needs of the look-ahead scratch arenas (doubles): the largest wave
inline void la_needs(const BatchPlan &P, const std::vector<LaNeed> &las, const std::vector<int> &la_of, size_t *part, size_t *small) {
    std::vector<size_t> wp(P.nwaves, 0), ws(P.nwaves, 0);
    for (size_t i = 0; i < P.cls.size(); i++)
        if (la_of[i] >= 0) { const LaLayout Y = la_layout(las[la_of[i]], P.with_u); wp[P.cls[i].wave] += Y.part_doubles; ws[P.cls[i].wave] += Y.small_doubles; }
    *part = *small = 0;
    for (int w = 0; w < P.nwaves; w++) { *part = std::max(*part, wp[w]); *small = std::max(*small, ws[w]); }
}

// The arena needs of a laid-out plan (doubles, from the plan's lane base on): the routes of its classes are chosen on the way
// (choose_routes: las / la_of as there).  raise: the running maximum over several plans.
struct PlanNeeds {
    size_t mat = 0, vec = 0, tab = 0, slab = 0, la_part = 0, la_small = 0;
    void raise(const PlanNeeds &o, size_t f = 1) {
        mat = std::max(mat, f * o.mat); vec = std::max(vec, f * o.vec); tab = std::max(tab, f * o.tab); slab = std::max(slab, f * o.slab);
        la_part = std::max(la_part, f * o.la_part); la_small = std::max(la_small, f * o.la_small);
    }
};
inline PlanNeeds plan_needs(const PlanRules &r, BatchPlan &P, std::vector<LaNeed> &las, std::vector<int> &la_of) {
    PlanNeeds nd{P.need_mat, P.need_vec, P.need_tab, P.need_slab, 0, 0};
    choose_routes(r, P, las, la_of);
    la_needs(P, las, la_of, &nd.la_part, &nd.la_small);
    return nd;
}

// End of the medgp_screen chunk that starts at entry e0 of the walk: entry e = (patient e / ninit of the walk, vector e % ninit); ns =
// the patients' sizes in walk order (largest first).  A chunk holds at most max_batch entries and at most screen_budget bytes of
// Gram matrices (8 ld^2 per entry: an nlml-only evaluation never forms U; ld taken at the upper end of the entry's size bucket, which
// bounds the leading dimension of whatever class it lands in).  Entries of >= 45 blocks (64 MB of matrix each) take the look-ahead
// schedule in any chunk this rule forms, and that schedule gains little beyond ~ 32 k block pairs per launch (measured on the four
// largest patients of the heavy-tailed cohort, N = 3258 .. 5832, 200 vectors each: 1234 / 1073 / 799 / 679 / 665 ms for chunks
// closed at 4 / 8 / 16 / 32 / 64 k block pairs, scratch/screen_work_sweep.sh): such a chunk is closed there or by the byte budget --
// N = 5832: 3 entries = 0.83 GB of matrices + 0.42 GB of scratch per chunk where round 5 took 32 entries = 26 GB + 9 GB (obtaining
// that much memory can cost seconds, see struct Arena in medgp_capi.hip).  The budget (2 GB) still gives every size its efficient route: 1024 entries of N <= 512 (one workgroup each, two per
// CU), 256 of N <= 1024 (one per CU), 64 of N <= 2048 (look-ahead schedule, saturated from 16 on).
inline size_t screen_chunk_end(const PlanRules &r, const std::vector<int> &ns, int ninit, size_t e0, size_t total, int max_entries) {
    size_t e = e0, bytes = 0;
    long long work = 0;
    while (e < total && (int)(e - e0) < max_entries) {
        const int nb = blocks64(ns[e / ninit]);
        const size_t ldb = (size_t)64 << size_bucket(nb), per = 8 * ldb * ldb;
        if (e > e0 && bytes + per > r.screen_budget) break;
        if (e > e0 && nb >= 45 && work >= r.screen_work) break;
        bytes += per; work += (long long)nb * nb; e++;
    }
    return e;
}

// How medgp_screen cuts `total` = walk_n.size() * ninit entries into chunks, whether it runs them on two lanes, and what ONE lane needs of
// every arena (doubles; the largest chunk, laid out once per distinct composition).  Shared with medgp_reserve_plan.
struct ScreenChunk { size_t e0, e1; };
struct ScreenCut {
    std::vector<ScreenChunk> chunks;
    bool two = false;
    int lane_rows = 0;
    size_t cap_mat = 0, cap_vec = 0, cap_tab = 0, cap_part = 0, cap_small = 0;
};
inline void screen_cut(const PlanRules &r, const std::vector<int> &walk_n, int ninit, ScreenCut &S) {
    const size_t total = walk_n.size() * (size_t)ninit;
    S.two = r.screen_lanes >= 2 && r.max_batch >= 2 && screen_chunk_end(r, walk_n, ninit, 0, total, r.max_batch) < total;
    S.lane_rows = S.two ? r.max_batch / 2 : r.max_batch;   // a lane's rows of the batch-indexed buffers = its chunks' entry cap
    S.chunks.clear();
    for (size_t e0 = 0; e0 < total;) { const size_t e = screen_chunk_end(r, walk_n, ninit, e0, total, S.lane_rows); S.chunks.push_back({e0, e}); e0 = e; }
    BatchPlan P;
    std::vector<LaNeed> las;
    std::vector<int> la_of, en;
    PlanNeeds cap{S.cap_mat, S.cap_vec, S.cap_tab, 0, S.cap_part, S.cap_small};
    int lf = -1, ll = -1;
    size_t lc = 0;
    for (const ScreenChunk &ch : S.chunks) {
        const int nf = walk_n[ch.e0 / ninit], nl = walk_n[(ch.e1 - 1) / ninit];
        if (nf == nl && nf == lf && nl == ll && ch.e1 - ch.e0 == lc) continue;   // (runs of identical chunks: laid out once)
        en.resize(ch.e1 - ch.e0);
        for (size_t x = ch.e0; x < ch.e1; x++) en[x - ch.e0] = walk_n[x / ninit];
        layout_plan(r, en.data(), (int)en.size(), false, P);
        cap.raise(plan_needs(r, P, las, la_of));
        lf = nf; ll = nl; lc = ch.e1 - ch.e0;
    }
    S.cap_mat = cap.mat; S.cap_vec = cap.vec; S.cap_tab = cap.tab; S.cap_part = cap.la_part; S.cap_small = cap.la_small;
}

// ---- per-entry result blocks, internal order -> the caller's rows -------------------------------------------------------------
// A call's kernels leave one block of `stride` doubles per entry, in the plan's internal order (entry i at src + i * stride).  A piece
// of the block -- `count` doubles from offset `off` -- is one row of a caller array `dst` of nbatch rows of `count` doubles (null: the
// caller did not ask for it).  Entry i is the caller's row order[i]; the rows of an entry whose status (the caller's order, as the
// calls return it) is negative are NaN.
struct BlockPiece { size_t off, count; double *dst; };
inline void scatter_entry_blocks(const int *order, const int *status, int nbatch, const double *src, size_t stride,
                                 std::initializer_list<BlockPiece> pieces) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < nbatch; i++) {
        const int b = order[i];
        for (const BlockPiece &p : pieces) {
            if (!p.dst) continue;
            double *row = p.dst + (size_t)b * p.count;
            if (status[b] >= 0) std::copy_n(src + (size_t)i * stride + p.off, p.count, row);
            else std::fill_n(row, p.count, nan);
        }
    }
}
