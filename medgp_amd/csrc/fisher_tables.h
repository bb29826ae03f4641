// fisher_tables.h -- host-side geometry of medgp_fisher_vec (kernels_fisher.h): the grids of its launches, the workgroup -> tile maps,
// the sizes of the call's own buffers and the capacity rule.  Plain C++ (the two tile maps are also compiled for the device): tested
// on the CPU by fisher_tables_test.cpp under sanitizers, so a geometry mistake shows there and not as an out-of-bounds access on a GPU.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define FISHER_HD __host__ __device__
#else
#define FISHER_HD
#endif

// matrices of ld^2 doubles the call holds per entry at once: K -> L -> P, U = L^-T, Kdot, T = P Kdot
#define FISHER_MATS 4

// k_fisher_t: one workgroup per tile (I, J) of ALL nt64 x nt64 tiles of the class's largest entry, row-major (T is not symmetric)
inline int fisher_t_grid(int nt64) { return nt64 * nt64; }
FISHER_HD inline void fisher_t_tile(int x, int nt64, int &I, int &J) {
    I = x / nt64;
    J = x - I * nt64;
}
// k_fisher_kdot: one workgroup per LOWER tile (I >= J), row by row; the tile and its mirror image are both stored
inline int fisher_kdot_grid(int nt64) { return nt64 * (nt64 + 1) / 2; }
FISHER_HD inline void fisher_lower_tile(int x, int &I, int &J) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= x) i++;
    I = i;
    J = x - i * (i + 1) / 2;
}

// doubles per entry of the direction's coefficient block, laid out like the hyper block k_prep leaves:
//   noise[D] | Bdot[Q D D] | cmu[Q] | cv[Q]
inline size_t fisher_coef_stride(int Q, int D) { return (size_t)D + (size_t)Q * D * D + 2 * (size_t)Q; }

struct FisherBuffers {
    size_t mat_doubles;    // each of Kdot and T: the plan's matrix need (every class laid out like Kmat)
    size_t coef_doubles;   // coefficient blocks of all entries
    size_t dir_doubles;    // each of the directions and the products on the device: nbatch * nvec * H
};
inline FisherBuffers fisher_buffers(size_t plan_need_mat, int nbatch, int nvec, int H, int Q, int D) {
    return FisherBuffers{plan_need_mat, (size_t)nbatch * fisher_coef_stride(Q, D), (size_t)nbatch * (size_t)nvec * (size_t)H};
}

// The capacity rule: the four matrices of every entry are alive at once (no memory waves), so they must fit the budget together.
// plan_need_mat: doubles of ONE matrix role over all entries of the call.
inline bool fisher_fits(size_t plan_need_mat, size_t mem_budget_bytes) {
    const size_t per = (size_t)FISHER_MATS * sizeof(double);
    return plan_need_mat <= mem_budget_bytes / per;
}
