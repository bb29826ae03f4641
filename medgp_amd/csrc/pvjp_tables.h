// pvjp_tables.h -- host-side geometry of medgp_posterior_vjp_batch (kernels_posterior_vjp.h): the by-covariate order of every
// patient's test points, the tile table, the per-entry records, the launch chunks (cut BETWEEN entries only: the work rows of all point
// tiles of an entry are resident for its product), the sizes of the call's own buffers and the capacity rules.  Plain C++ (no HIP
// header, no kernel): tested on the CPU by pvjp_tables_test.cpp under sanitizers, so a geometry mistake shows there and not as an
// out-of-bounds access on a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>
#include "pjvp_tables.h"

// matrices of ld^2 doubles the call holds per entry at once: K -> L, U = L^-T (G never reaches memory, no Kdot)
#define PVJP_MATS 2

// one entry of the call (internal order): its index (row of pseg), the first of its tiles inside its launch chunk (work rows), its
// points [p0, p0 + m) of the call in the device's order
struct PvjpEnt { int ent, tile0, p0, m; };
// a launch chunk: entries [e0, e0 + ne) of class cls, tiles [t0, t0 + nt) of the tile table, `stride` doubles of work rows per tile
struct PvjpChunk { int cls, e0, ne, t0, nt; size_t stride; };

struct PvjpTables {
    std::vector<int64_t> src;      // device point k is the caller's point src[k] (inside every patient: stably sorted by covariate)
    std::vector<int> dev_of;       // caller point -> device point
    std::vector<int> pseg;         // [internal entry][D + 1]: the covariate ranges of its points, relative to its first point
    std::vector<PostTile> tiles;   // PostTile::e counts inside the class, as k_pjvp_solve takes it
    std::vector<PvjpEnt> ents;     // [internal entry]
    std::vector<PvjpChunk> chunks;
    size_t work_need = 0;          // bytes of work rows of the largest chunk
};

// meta2: the points' covariates in [0, D) (checked by the caller), or null (all points of covariate 0).  False: entry err.entry
// (caller index err.b) alone needs err.need bytes of work rows, more than the budget.
inline bool build_pvjp_tables(const std::vector<TableClass> &cls, const int *order, const int64_t *offsets, const int32_t *meta2, int nbatch,
                              int D, size_t budget, PvjpTables &T, TableError &err) {
    const int64_t M = offsets[nbatch];
    T.src.resize((size_t)M);
    T.dev_of.resize((size_t)M);
    T.pseg.assign((size_t)nbatch * (D + 1), 0);
    T.ents.assign((size_t)nbatch, PvjpEnt{0, 0, 0, 0});
    std::iota(T.src.begin(), T.src.end(), (int64_t)0);
    for (int b = 0; b < nbatch; b++)
        if (meta2) std::stable_sort(T.src.begin() + offsets[b], T.src.begin() + offsets[b + 1], [&](int64_t x, int64_t y) { return meta2[x] < meta2[y]; });
    for (int64_t k = 0; k < M; k++) T.dev_of[(size_t)T.src[(size_t)k]] = (int)k;
    for (size_t ci = 0; ci < cls.size(); ci++) {
        const TableClass &k = cls[ci];
        const size_t stride = pjvp_work_stride(k.ld);
        PvjpChunk ch{(int)ci, 0, 0, (int)T.tiles.size(), 0, stride};
        auto close = [&]() {
            if (ch.ne > 0) {
                T.chunks.push_back(ch);
                T.work_need = std::max(T.work_need, (size_t)ch.nt * stride * sizeof(double));
            }
            ch = PvjpChunk{(int)ci, ch.e0 + ch.ne, 0, (int)T.tiles.size(), 0, stride};
        };
        for (int i = k.b0; i < k.b0 + k.count; i++) {
            const int b = order[i];
            const int64_t m = offsets[b + 1] - offsets[b];
            const int nt = (int)((m + POST_TW - 1) / POST_TW);
            const size_t need = (size_t)nt * stride * sizeof(double);
            if (need > budget) { err = {b, i, -1, (long long)m, need}; return false; }
            if ((size_t)ch.nt * stride * sizeof(double) + need > budget) close();
            T.ents[(size_t)i] = PvjpEnt{i, ch.nt, (int)offsets[b], (int)m};
            int *ps = T.pseg.data() + (size_t)i * (D + 1);
            for (int64_t p = offsets[b]; p < offsets[b + 1]; p++) ps[(meta2 ? meta2[T.src[(size_t)p]] : 0) + 1]++;
            for (int d = 0; d < D; d++) ps[d + 1] += ps[d];
            push_point_tiles(T.tiles, i - k.b0, offsets[b], offsets[b + 1], nullptr);
            ch.nt += nt;
            ch.ne++;
        }
        close();
    }
    return true;
}

struct PvjpBuffers {
    size_t in_doubles;      // [cot_mean ncot M | cot_var ncot M | y2 M | wt M]
    size_t pts_doubles;     // [cm M | cv M | l M | cos Q M | sin Q M | mean M | var M]
    size_t vec_doubles;     // c = W cm: the plan's vector need (laid out like alpha)
    size_t small_doubles;   // per entry [sum cv D | loss | -]
    size_t out_doubles;     // the gradients, set-major [ncot][nbatch][H] (k_epilogue's row stride is H)
};
inline size_t pvjp_mz(int64_t M) { return (size_t)(M > 0 ? M : 1); }
// where the fp64 mean starts in the per-point buffer (var: Mz further)
inline size_t pvjp_moments_offset(int Q, int64_t M) { return (3 + 2 * (size_t)Q) * pvjp_mz(M); }
inline PvjpBuffers pvjp_buffers(size_t plan_need_vec, int nbatch, int ncot, int H, int Q, int D, int64_t M) {
    const size_t Mz = pvjp_mz(M);
    return PvjpBuffers{(2 * (size_t)ncot + 2) * Mz, (5 + 2 * (size_t)Q) * Mz, std::max<size_t>(plan_need_vec, 1), (size_t)nbatch * (D + 2),
                       (size_t)ncot * nbatch * H};
}
// grid x of k_pvjp_cross: four lower bins per workgroup
inline int pvjp_cross_grid(int D) { return (D * (D + 1) / 2 + 3) / 4; }

// The capacity rule: the two matrices of every entry are alive at once (no memory waves).  plan_need_mat: doubles of ONE matrix role.
inline bool pvjp_fits(size_t plan_need_mat, size_t mem_budget_bytes) {
    const size_t per = (size_t)PVJP_MATS * sizeof(double);
    return plan_need_mat <= mem_budget_bytes / per;
}
