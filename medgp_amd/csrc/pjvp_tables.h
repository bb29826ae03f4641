// pjvp_tables.h -- host-side geometry of medgp_posterior_jvp_batch (kernels_posterior_jvp.h): the tile table and the launch chunks of
// its test points, the sizes of the call's own buffers, the grids of its launches and the capacity rule.  Plain C++ (no HIP header, no
// kernel): tested on the CPU by pjvp_tables_test.cpp under sanitizers, so a geometry mistake shows there and not as an out-of-bounds
// access on a GPU.  Kdot and the coefficient blocks take the Fisher call's maps (fisher_tables.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include "fisher_tables.h"
#include "inference_tables.h"

// matrices of ld^2 doubles the call holds per entry at once: K -> L, U = L^-T, Kdot
#define PJVP_MATS 3
// panels of ld x 64 doubles in a tile's work rows: K* -> W = P K*, and V = L^-1 K*
#define PJVP_WORK_PANELS 2

// doubles of work rows of one tile of a class with leading dimension ld
inline size_t pjvp_work_stride(int ld) { return (size_t)PJVP_WORK_PANELS * (size_t)ld * 64; }

// The tile table per size class (POST_TW points per tile, the posterior call's PostTile) and chunks of consecutive tiles of one class
// whose work rows stay within the budget (a chunk holds at least one tile).  The chunks of a class are consecutive in T.chunks.
inline void build_pjvp_tiles(const std::vector<TableClass> &cls, const int *order, const int64_t *offsets, size_t budget,
                             PointTables<PostTile> &T) {
    for (size_t ci = 0; ci < cls.size(); ci++) {
        const TableClass &k = cls[ci];
        const int t_begin = (int)T.tiles.size();
        const size_t stride = pjvp_work_stride(k.ld);
        for (int i = k.b0; i < k.b0 + k.count; i++) push_point_tiles(T.tiles, i - k.b0, offsets[order[i]], offsets[order[i] + 1], nullptr);
        const int per_chunk = (int)std::max<size_t>(1, budget / (stride * sizeof(double)));
        for (int t0 = t_begin; t0 < (int)T.tiles.size(); t0 += per_chunk) {
            const int nt = std::min(per_chunk, (int)T.tiles.size() - t0);
            T.chunks.push_back({(int)ci, t0, nt, stride, 0, 0, 0, 0, 0, 0});
            T.work_need = std::max(T.work_need, (size_t)nt * stride * sizeof(double));
        }
    }
}

// k_pjvp_u: one workgroup per 64 rows of the class's largest entry
inline int pjvp_u_grid(int nt64) { return nt64; }

struct PjvpBuffers {
    size_t mat_doubles;    // Kdot: the plan's matrix need (every class laid out like Kmat)
    size_t coef_doubles;   // coefficient blocks of all entries (k_fisher_prep)
    size_t dir_doubles;    // the directions on the device: nbatch * nvec * H
    size_t u_doubles;      // u = Kdot alpha: the plan's vector need (every class laid out like alpha)
    size_t out_doubles;    // [dmean | dvar], each M * nvec (at least one double each)
};
inline PjvpBuffers pjvp_buffers(size_t plan_need_mat, size_t plan_need_vec, int nbatch, int nvec, int H, int Q, int D, int64_t M) {
    const FisherBuffers fb = fisher_buffers(plan_need_mat, nbatch, nvec, H, Q, D);
    const size_t per = (size_t)(M > 0 ? M : 1) * (size_t)nvec;
    return PjvpBuffers{fb.mat_doubles, fb.coef_doubles, fb.dir_doubles, plan_need_vec, 2 * per};
}
// where dvar starts in the output buffer
inline size_t pjvp_dvar_offset(int64_t M, int nvec) { return (size_t)(M > 0 ? M : 1) * (size_t)nvec; }

// The capacity rule: the three matrices of every entry are alive at once (no memory waves), so they must fit the budget together.
// plan_need_mat: doubles of ONE matrix role over all entries of the call.
inline bool pjvp_fits(size_t plan_need_mat, size_t mem_budget_bytes) {
    const size_t per = (size_t)PJVP_MATS * sizeof(double);
    return plan_need_mat <= mem_budget_bytes / per;
}
