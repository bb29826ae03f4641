// inference_tables.h -- the launch tables of the inference entry points (posterior, joint posterior, forecast, LOO) and the host
// arithmetic that builds them: which points a tile owns, where a launch chunk is cut, where a patient's or a group's block starts.
// Plain C++ on plain data (no HIP header, no kernel): the kernel headers include it for the table structs, medgp_capi.hip for the
// builders, and inference_tables_test.cpp compiles it alone with the host compiler, under sanitizers, against brute-force restatements.
// Inputs of the builders: the size classes of the call's plan (TableClass; internal entries [b0, b0 + count) share the leading dimension
// ld), order[i] = caller index of internal entry i, and per-caller-entry prefix arrays (offsets: test points; ooff / goff: observations /
// groups).  `budget` is the bytes one launch chunk may hold (MEDGP_POSTERIOR_BUDGET_GB).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__HIP__)
#define MEDGP_HD __host__ __device__
#else
#define MEDGP_HD
#endif

#define POST_TW 64    // test points per tile (one workgroup)
#define TREND_TW 32   // test points per tile of k_trend: the tile's 64 columns hold the value and the slope column of each point

// one workgroup of k_posterior: entry e of the class view, test points [p0, p0 + cnt) of the call (cnt <= POST_TW)
struct PostTile { int e, p0, cnt, pad; };
// one workgroup of k_forecast: entry e of the class view, points [p0, p0 + cnt) of the call in the call's SORTED order
// (cnt <= POST_TW), pmax = the largest prefix among them
struct ForeTile { int e, p0, cnt, pmax; };
// one patient of a joint call
struct JointPat {
    int e;             // entry of the class view
    int b;             // caller index (cov_status row)
    int p0, m;         // its test points [p0, p0 + m) of the call
    int tile0;         // first of its tiles in the launch chunk (work rows)
    int pad;
    long long coff;    // offset (doubles) of its C (mpad x mpad, mpad = m rounded up to 64) in the chunk's C buffer
    long long voff;    // offset (floats) of its m x m block in the chunk's cov buffer
};
// one workgroup of k_postcov: tile pair (I, J), I >= J, of patient pat; of k_postdraw: row block I (J unused)
struct JointTile { int pat, I, J, pad; };
// one singleton group of a LOO call
struct LooSingle {
    int e;     // entry of the class view
    int r;     // its row of the entry (internal order)
    int out;   // its observation of the call (mean / var, the caller's order)
    int g;     // its group of the call (lpd)
};
// one member of a larger group: the index list of a group is rows[p0 .. p0 + m), r ascending
struct LooRow { int r, out; };
// A larger group is a JointPat: e = entry of the class view, b = its group of the call (lpd / group_status row), p0 = first of its
// rows in the index list, m = its size, coff = offset (doubles) of its block in the chunk's buffer:
//   [mpad x mpad] M -> R | [mpad x mpad] R^-1 (k_loo_solve's panels) | [mpad] w | [mpad] R^-T w,     mpad = m rounded up to 64.
// A workgroup of k_loo_gram is a JointTile (pat, I, J), I >= J; of k_loo_solve (pat, I = column tile, J = 0) or (pat, 0, J = 1: the
// vector solves).
MEDGP_HD inline size_t loo_block_doubles(int m) {
    const size_t mpad = ((size_t)m + 63) / 64 * 64;
    return 2 * mpad * mpad + 2 * mpad;
}

struct TableClass { int b0, count, ld; };
// a launch chunk: tiles [t0, t0 + nt) of class cls, `stride` doubles of work rows per tile; a joint call's chunk also has its
// patients [pat0, pat0 + npat), tile pairs and row blocks
struct TileChunk { int cls, t0, nt; size_t stride; int pat0, npat, pair0, npair, blk0, nblk; };
// what did not fit the budget: caller entry b (internal entry `entry`), group gid (LOO), m points / members, `need` bytes at once
struct TableError { int b, entry, gid; long long m; size_t need; };

template <class Tile>
struct PointTables {
    std::vector<Tile> tiles;
    std::vector<TileChunk> chunks;
    size_t work_need = 0;   // bytes of work rows of the largest chunk
};

// the tiles of points [p0, p1) of entry e, tw points each; prefix (the points' prefixes, sorted ascending inside the patient) fills pmax
template <class Tile>
inline void push_point_tiles(std::vector<Tile> &tiles, int e, int64_t p0, int64_t p1, const int *prefix, int tw = POST_TW) {
    for (int64_t p = p0; p < p1; p += tw) {
        const int cnt = (int)std::min<int64_t>(tw, p1 - p);
        tiles.push_back({e, (int)p, cnt, prefix ? prefix[p + cnt - 1] : 0});   // (sorted: the tile's last point has its largest prefix)
    }
}

// medgp_posterior_batch / medgp_forecast_batch: the tile table per size class (entries of a class share the view's leading dimension,
// hence the work-row stride ld * 64 + extra doubles) and chunks of consecutive tiles of one class whose work rows stay within the budget
template <class Tile>
inline void build_point_tiles(const std::vector<TableClass> &cls, const int *order, const int64_t *offsets, const int *prefix,
                              size_t extra, size_t budget, PointTables<Tile> &T, int tw = POST_TW) {
    for (size_t ci = 0; ci < cls.size(); ci++) {
        const TableClass &k = cls[ci];
        const int t_begin = (int)T.tiles.size();
        const size_t stride = (size_t)k.ld * 64 + extra;
        for (int i = k.b0; i < k.b0 + k.count; i++) push_point_tiles(T.tiles, i - k.b0, offsets[order[i]], offsets[order[i] + 1], prefix, tw);
        const int per_chunk = (int)std::max<size_t>(1, budget / (stride * sizeof(double)));
        for (int t0 = t_begin; t0 < (int)T.tiles.size(); t0 += per_chunk) {
            const int nt = std::min(per_chunk, (int)T.tiles.size() - t0);
            T.chunks.push_back({(int)ci, t0, nt, stride, 0, 0, 0, 0, 0, 0});
            T.work_need = std::max(T.work_need, (size_t)nt * stride * sizeof(double));
        }
    }
}

// medgp_trend_batch: the posterior call's tables with TREND_TW points per tile.  A tile's work rows are still ld x 64 doubles: its 64
// columns are the value and the slope columns of its points (kernels_trend.h).
inline void build_trend_tiles(const std::vector<TableClass> &cls, const int *order, const int64_t *offsets, size_t budget,
                              PointTables<PostTile> &T) {
    build_point_tiles(cls, order, offsets, nullptr, 0, budget, T, TREND_TW);
}

// medgp_components_batch: the 64 columns of a tile are the Q component columns of 64 / Q points (kernels_components.h; Q <= 64)
MEDGP_HD inline int components_tw(int Q) { return 64 / Q; }
// doubles of a tile beyond its ld x 64 work rows: the running sums of its (64 / Q) Q (Q - 1) / 2 component pairs (at most 2016)
MEDGP_HD inline size_t components_extra(int Q, bool with_cov) { return with_cov ? (size_t)components_tw(Q) * ((size_t)Q * (Q - 1) / 2) : 0; }
// the posterior call's tables with that many points per tile and those extra doubles
inline void build_components_tiles(const std::vector<TableClass> &cls, const int *order, const int64_t *offsets, int Q, bool with_cov,
                                   size_t budget, PointTables<PostTile> &T) {
    build_point_tiles(cls, order, offsets, nullptr, components_extra(Q, with_cov), budget, T, components_tw(Q));
}

// medgp_functional_batch: the two-level CSR of a call -- patient b owns functionals [foffsets[b], foffsets[b + 1]), functional f owns
// terms [toffsets[f], toffsets[f + 1]) -- checked before anything is read through it.  The error kinds, in the order they are looked for:
enum FunctionalCsrError {
    FUNC_CSR_OK = 0,
    FUNC_CSR_NULL,          // foffsets or toffsets is null (toffsets is required even for a call without functionals: toffsets[0])
    FUNC_CSR_FIRST,         // foffsets[0] != 0                                (at = 0)
    FUNC_CSR_DECREASE,      // foffsets[at + 1] < foffsets[at]
    FUNC_CSR_COUNT,         // more than FUNC_MAX_FUNCTIONALS functionals
    FUNC_CSR_TERM_FIRST,    // toffsets[0] != 0                                (at = 0)
    FUNC_CSR_TERM_DECREASE, // toffsets[at + 1] < toffsets[at]
    FUNC_CSR_TERM_COUNT     // more than FUNC_MAX_TERMS terms                  (at = the functional that passes it)
};
#define FUNC_TW 64                                        // functionals per tile of k_functional: one solve column each
#define FUNC_MAX_FUNCTIONALS ((int64_t)INT32_MAX - FUNC_TW)   // a tile's p0 + cnt and the offset table of F + 1 ints stay in int
#define FUNC_MAX_TERMS ((int64_t)INT32_MAX)
// what the entry point stages of a checked call: F functionals, T terms, toff [F + 1] the term offsets as the device's ints, fun [T]
// the functional of every term
struct FunctionalCsr {
    int64_t F = 0, T = 0, at = -1;   // at: where the error was found (FunctionalCsrError)
    std::vector<int> toff, fun;
};
// Nothing behind a broken place is read: foffsets is walked first (nbatch + 1 values), toffsets only up to foffsets[nbatch] + 1 values
// of a foffsets found sound, and the walk stops at the first violation.
inline FunctionalCsrError check_functional_csr(const int64_t *foffsets, const int64_t *toffsets, int nbatch, FunctionalCsr &out) {
    out = FunctionalCsr{};
    if (!foffsets || !toffsets) return FUNC_CSR_NULL;
    if (foffsets[0] != 0) { out.at = 0; return FUNC_CSR_FIRST; }
    for (int b = 0; b < nbatch; b++)
        if (foffsets[b + 1] < foffsets[b]) { out.at = b; return FUNC_CSR_DECREASE; }
    const int64_t F = foffsets[nbatch];
    if (F > FUNC_MAX_FUNCTIONALS) { out.at = nbatch; return FUNC_CSR_COUNT; }
    if (toffsets[0] != 0) { out.at = 0; return FUNC_CSR_TERM_FIRST; }
    for (int64_t f = 0; f < F; f++) {
        if (toffsets[f + 1] < toffsets[f]) { out.at = f; return FUNC_CSR_TERM_DECREASE; }
        if (toffsets[f + 1] > FUNC_MAX_TERMS) { out.at = f; return FUNC_CSR_TERM_COUNT; }
    }
    out.F = F;
    out.T = toffsets[F];
    out.toff.resize((size_t)F + 1);
    out.fun.resize((size_t)out.T);
    for (int64_t f = 0; f <= F; f++) out.toff[(size_t)f] = (int)toffsets[f];
    for (int64_t f = 0; f < F; f++)
        for (int64_t x = toffsets[f]; x < toffsets[f + 1]; x++) out.fun[(size_t)x] = (int)f;
    return FUNC_CSR_OK;
}
// The internal position of every functional after the plan's reordering of the entries: pos[f] = the rank of functional f when the
// classes are walked in order, their entries in internal order and each patient's functionals in the caller's.  The tile table walks
// the functionals in exactly this order (tile k of build_functional_tiles owns FUNC_TW consecutive positions of one patient), while
// its p0 keeps the caller's numbering: the outputs need no scatter.
inline void functional_positions(const std::vector<TableClass> &cls, const int *order, const int64_t *foffsets, std::vector<int64_t> &pos) {
    int64_t F = 0, next = 0;
    for (const TableClass &k : cls)
        for (int i = k.b0; i < k.b0 + k.count; i++) F = std::max(F, foffsets[order[i] + 1]);
    pos.assign((size_t)F, -1);
    for (const TableClass &k : cls)
        for (int i = k.b0; i < k.b0 + k.count; i++)
            for (int64_t f = foffsets[order[i]]; f < foffsets[order[i] + 1]; f++) pos[(size_t)f] = next++;
}
// the posterior call's tables over the functionals: FUNC_TW per tile (kernels_functional.h), nothing behind a tile's ld x 64 work rows
inline void build_functional_tiles(const std::vector<TableClass> &cls, const int *order, const int64_t *foffsets, size_t budget,
                                   PointTables<PostTile> &T) {
    build_point_tiles(cls, order, foffsets, nullptr, 0, budget, T, FUNC_TW);
}

struct JointTables : PointTables<PostTile> {
    std::vector<JointPat> pats;
    std::vector<JointTile> pairs, blks;
    size_t c_need = 0, cov_need = 0;   // bytes of C / of the float covariance blocks of the largest chunk
};

// medgp_posterior_joint_batch: chunks of WHOLE patients (the work rows of all tiles of a patient, its C and its float block of cov are
// resident at once), with the patient / tile-pair / row-block tables.  false: one patient alone exceeds the budget (err).
inline bool build_joint_chunks(const std::vector<TableClass> &cls, const int *order, const int64_t *offsets, size_t extra, bool want_cov,
                               size_t budget, JointTables &T, TableError &err) {
    for (size_t ci = 0; ci < cls.size(); ci++) {
        const TableClass &k = cls[ci];
        const size_t stride = (size_t)k.ld * 64 + extra;
        TileChunk ch{(int)ci, (int)T.tiles.size(), 0, stride, (int)T.pats.size(), 0, (int)T.pairs.size(), 0, (int)T.blks.size(), 0};
        size_t wbytes = 0, cdbl = 0, cflt = 0;
        auto close = [&]() {
            if (ch.npat == 0) return;
            T.chunks.push_back(ch);
            T.work_need = std::max(T.work_need, wbytes); T.c_need = std::max(T.c_need, cdbl * sizeof(double)); T.cov_need = std::max(T.cov_need, cflt * sizeof(float));
            ch.t0 += ch.nt; ch.nt = 0; ch.pat0 += ch.npat; ch.npat = 0; ch.pair0 += ch.npair; ch.npair = 0; ch.blk0 += ch.nblk; ch.nblk = 0;
            wbytes = cdbl = cflt = 0;
        };
        for (int i = k.b0; i < k.b0 + k.count; i++) {
            const int b = order[i];
            const int64_t m = offsets[b + 1] - offsets[b];
            if (m == 0) continue;
            const int nt = (int)((m + POST_TW - 1) / POST_TW);
            const size_t mpad = (size_t)nt * 64;
            // V of all its tiles, C, and its float block of cov
            const size_t need = (size_t)nt * stride * sizeof(double) + mpad * mpad * sizeof(double) + (want_cov ? (size_t)m * m * sizeof(float) : 0);
            if (need > budget) { err = {b, i, -1, (long long)m, need}; return false; }
            if (wbytes + cdbl * sizeof(double) + cflt * sizeof(float) + need > budget) close();
            const int pidx = (int)T.pats.size();
            T.pats.push_back({i - k.b0, b, (int)offsets[b], (int)m, ch.nt, 0, (long long)cdbl, (long long)cflt});
            push_point_tiles(T.tiles, i - k.b0, offsets[b], offsets[b + 1], nullptr);
            for (int I = 0; I < nt; I++) {
                for (int J = 0; J <= I; J++) T.pairs.push_back({pidx, I, J, 0});
                T.blks.push_back({pidx, I, 0, 0});
            }
            ch.nt += nt; ch.npat++; ch.npair += nt * (nt + 1) / 2; ch.nblk += nt;
            wbytes += (size_t)nt * stride * sizeof(double); cdbl += mpad * mpad; if (want_cov) cflt += (size_t)m * m;
        }
        close();
    }
    return true;
}

// medgp_functional_joint_batch: the joint call's chunks over the FUNCTIONALS of a patient -- whole patients per chunk (the work rows of
// all its tiles of FUNC_TW functionals and its F x F float block of fcov are resident at once; no fp64 C: nothing is factored), with the
// patient table (JointPat: p0 = its first functional of the call, m = F, coff unused) and the lower tile pairs of k_funccov; no row
// blocks.  The tiles are those of build_functional_tiles, in its order; a patient without functionals has no tile, no pair and no
// JointPat.  false: one patient alone exceeds the budget (err).
inline bool build_functional_joint_chunks(const std::vector<TableClass> &cls, const int *order, const int64_t *foffsets, size_t budget,
                                          JointTables &T, TableError &err) {
    for (size_t ci = 0; ci < cls.size(); ci++) {
        const TableClass &k = cls[ci];
        const size_t stride = (size_t)k.ld * 64;
        TileChunk ch{(int)ci, (int)T.tiles.size(), 0, stride, (int)T.pats.size(), 0, (int)T.pairs.size(), 0, 0, 0};
        size_t wbytes = 0, cflt = 0;
        auto close = [&]() {
            if (ch.npat == 0) return;
            T.chunks.push_back(ch);
            T.work_need = std::max(T.work_need, wbytes); T.cov_need = std::max(T.cov_need, cflt * sizeof(float));
            ch.t0 += ch.nt; ch.nt = 0; ch.pat0 += ch.npat; ch.npat = 0; ch.pair0 += ch.npair; ch.npair = 0;
            wbytes = cflt = 0;
        };
        for (int i = k.b0; i < k.b0 + k.count; i++) {
            const int b = order[i];
            const int64_t F = foffsets[b + 1] - foffsets[b];
            if (F == 0) continue;
            const int nt = (int)((F + FUNC_TW - 1) / FUNC_TW);
            // V of all its tiles and its float block of fcov (F <= FUNC_MAX_FUNCTIONALS: F^2 floats stay in size_t)
            const size_t vbytes = (size_t)nt * stride * sizeof(double), fbytes = (size_t)F * (size_t)F * sizeof(float);
            if (fbytes > budget || vbytes > budget - fbytes) { err = {b, i, -1, (long long)F, vbytes + fbytes}; return false; }
            if (wbytes + cflt * sizeof(float) + vbytes + fbytes > budget) close();
            const int pidx = (int)T.pats.size();
            T.pats.push_back({i - k.b0, b, (int)foffsets[b], (int)F, ch.nt, 0, 0, (long long)cflt});
            push_point_tiles(T.tiles, i - k.b0, foffsets[b], foffsets[b + 1], nullptr, FUNC_TW);
            for (int I = 0; I < nt; I++)
                for (int J = 0; J <= I; J++) T.pairs.push_back({pidx, I, J, 0});
            ch.nt += nt; ch.npat++; ch.npair += nt * (nt + 1) / 2;
            wbytes += vbytes; cflt += (size_t)F * (size_t)F;
        }
        close();
    }
    return true;
}

// a launch chunk of medgp_loo_batch: groups [g0, g0 + ng) of class cls with their tile pairs and solve jobs
struct LooChunk { int cls, g0, ng, pair0, npair, job0, njob; };
struct LooClassSingles { int cls, s0, ns; };
struct LooTables {
    std::vector<LooSingle> singles;
    std::vector<LooClassSingles> csing;   // every class's singletons [s0, s0 + ns)
    std::vector<LooRow> rows;
    std::vector<JointPat> groups;
    std::vector<JointTile> pairs, jobs;
    std::vector<LooChunk> chunks;
    std::vector<int> gsize;               // members of every group of the call
    size_t blk_need = 0;                  // bytes of blocks of the largest chunk
};

// medgp_loo_batch: per size class its singletons; chunks of larger groups (whole groups, blocks within the budget) with their tile
// pairs and solve jobs -- one workgroup per table row, so ragged groups cost no idle workgroups.  en[i] = n of internal entry i;
// ooff / goff: first observation / first group of caller entry b in the call; group: the caller's group ids (null: every observation
// its own group); perm[b]: internal row -> caller observation of entry b (null: identity).  Jobs: one per column tile when the
// variances are wanted (want_var), one for the vector solves when mean or lpd are (want_vec).  false: one group alone exceeds the budget.
inline bool build_loo_tables(const std::vector<TableClass> &cls, const int *order, const int *en, const int64_t *ooff, const int64_t *goff,
                             int nbatch, const int32_t *group, const int *const *perm, bool want_var, bool want_vec, size_t budget,
                             LooTables &T, TableError &err) {
    T.gsize.assign((size_t)goff[nbatch], 0);
    std::vector<int> cnt, start, fill;
    for (size_t ci = 0; ci < cls.size(); ci++) {
        const TableClass &k = cls[ci];
        const int s0 = (int)T.singles.size();
        LooChunk ch{(int)ci, (int)T.groups.size(), 0, (int)T.pairs.size(), 0, (int)T.jobs.size(), 0};
        size_t cdbl = 0;
        auto close = [&]() {
            if (ch.ng == 0) return;
            T.chunks.push_back(ch);
            T.blk_need = std::max(T.blk_need, cdbl * sizeof(double));
            ch.g0 += ch.ng; ch.ng = 0; ch.pair0 += ch.npair; ch.npair = 0; ch.job0 += ch.njob; ch.njob = 0;
            cdbl = 0;
        };
        for (int i = k.b0; i < k.b0 + k.count; i++) {
            const int b = order[i], n = en[i], G = (int)(goff[b + 1] - goff[b]);
            auto gid_of = [&](int r, int *cobs) { *cobs = perm[b] ? perm[b][r] : r; return group ? group[ooff[b] + *cobs] : *cobs; };
            cnt.assign(G, 0); start.assign(G, -1); fill.assign(G, 0);
            int co;
            for (int r = 0; r < n; r++) { const int gid = gid_of(r, &co); if (gid >= 0) cnt[gid]++; }
            for (int gid = 0; gid < G; gid++) {
                T.gsize[goff[b] + gid] = cnt[gid];
                if (cnt[gid] < 2) continue;
                const size_t need = loo_block_doubles(cnt[gid]) * sizeof(double);
                if (need > budget) { err = {b, i, gid, cnt[gid], need}; return false; }
                if (cdbl * sizeof(double) + need > budget) close();
                const int gidx = (int)T.groups.size(), nt = (cnt[gid] + 63) / 64;
                start[gid] = (int)T.rows.size();
                T.rows.resize(T.rows.size() + cnt[gid]);
                T.groups.push_back({i - k.b0, (int)(goff[b] + gid), start[gid], cnt[gid], 0, 0, (long long)cdbl, 0});
                for (int I = 0; I < nt; I++)
                    for (int J = 0; J <= I; J++) T.pairs.push_back({gidx, I, J, 0});
                int nj = 0;
                if (want_var) for (int I = 0; I < nt; I++, nj++) T.jobs.push_back({gidx, I, 0, 0});
                if (want_vec) { T.jobs.push_back({gidx, 0, 1, 0}); nj++; }
                ch.ng++; ch.npair += nt * (nt + 1) / 2; ch.njob += nj;
                cdbl += loo_block_doubles(cnt[gid]);
            }
            for (int r = 0; r < n; r++) {   // (rows ascending: the index list of a group is sorted, stably)
                const int gid = gid_of(r, &co);
                if (gid < 0) continue;
                if (cnt[gid] == 1) T.singles.push_back({i - k.b0, r, (int)(ooff[b] + co), (int)(goff[b] + gid)});
                else T.rows[start[gid] + fill[gid]++] = {r, (int)(ooff[b] + co)};
            }
        }
        close();
        T.csing.push_back({(int)ci, s0, (int)T.singles.size() - s0});
    }
    return true;
}

// medgp_lgo_grad: what its own kernels need beyond the tables of build_loo_tables (T, built with want_var = false, want_vec = true).
// Per launch chunk of T (chunks[i] belongs to T.chunks[i]) one workgroup per row:
//   cols   (group, I = 64-column tile of R^-1)                          k_lgo_inv
//   trows  (group, I = 64-row block of the group's ENTRY)               k_lgo_t: the rows of P that take part in P[:, B_g] S_g
// `pat` of a row is the group's index in T.groups, as in T.pairs.  And per entry:
//   sgl    ld ints per entry, class after class (sgl_off[ci] = first int of class ci), entry after entry: the group of the call that
//          row r is as a singleton, -1 for every other row (a member of a larger group, id -1, padding)
//   gord   the non-empty groups of the call, entry after entry (internal order), those of an entry by their FIRST member's row: the
//          order in which J adds the lpd of an entry's groups -- it does not depend on the labels
//   ent    two ints per internal entry i: its range [x0, x1) of gord
struct LgoChunk { int col0, ncol, trow0, ntrow; };
struct LgoTables {
    std::vector<JointTile> cols, trows;
    std::vector<LgoChunk> chunks;
    std::vector<int> sgl, gord, ent;
    std::vector<size_t> sgl_off;
};
inline void build_lgo_tables(const std::vector<TableClass> &cls, const int *en, const LooTables &T, LgoTables &G) {
    size_t total = 0;
    int nent = 0;
    for (const TableClass &k : cls) { G.sgl_off.push_back(total); total += (size_t)k.count * k.ld; nent = std::max(nent, k.b0 + k.count); }
    G.sgl.assign(total, -1);
    G.ent.assign(2 * (size_t)nent, 0);
    std::vector<std::vector<std::pair<int, int>>> first((size_t)nent);   // per internal entry (first row, group of the call)
    for (const LooClassSingles &s : T.csing)
        for (int x = s.s0; x < s.s0 + s.ns; x++) {
            const LooSingle &S = T.singles[(size_t)x];
            const TableClass &k = cls[(size_t)s.cls];
            G.sgl[G.sgl_off[(size_t)s.cls] + (size_t)S.e * k.ld + S.r] = S.g;
            first[(size_t)(k.b0 + S.e)].push_back({S.r, S.g});
        }
    for (const LooChunk &ch : T.chunks)
        for (int gi = ch.g0; gi < ch.g0 + ch.ng; gi++) {
            const JointPat &P = T.groups[(size_t)gi];
            first[(size_t)(cls[(size_t)ch.cls].b0 + P.e)].push_back({T.rows[(size_t)P.p0].r, P.b});
        }
    for (int i = 0; i < nent; i++) {
        std::sort(first[(size_t)i].begin(), first[(size_t)i].end());
        G.ent[2 * (size_t)i] = (int)G.gord.size();
        for (const auto &fg : first[(size_t)i]) G.gord.push_back(fg.second);
        G.ent[2 * (size_t)i + 1] = (int)G.gord.size();
    }
    for (const LooChunk &ch : T.chunks) {
        const TableClass &k = cls[(size_t)ch.cls];
        LgoChunk c{(int)G.cols.size(), 0, (int)G.trows.size(), 0};
        for (int gi = ch.g0; gi < ch.g0 + ch.ng; gi++) {
            const JointPat &P = T.groups[(size_t)gi];
            const int nt = (P.m + 63) / 64, nrb = (std::max(en[k.b0 + P.e], 1) + 63) / 64;
            for (int I = 0; I < nt; I++) G.cols.push_back({gi, I, 0, 0});
            for (int rb = 0; rb < nrb; rb++) G.trows.push_back({gi, rb, 0, 0});
            c.ncol += nt; c.ntrow += nrb;
        }
        G.chunks.push_back(c);
    }
}
