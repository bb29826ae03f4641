// hess_tables.h -- host-side geometry of medgp_hess_vec (kernels_hess.h): the sizes and offsets of the call's own buffers, the grids
// of its launches and the capacity rule.  Plain C++ (the slab stride is also compiled for the device): tested on the CPU by
// hess_tables_test.cpp under sanitizers, so a geometry mistake shows there and not as an out-of-bounds access on a GPU.
// The tile launches (k_hess_moments, k_hess_wgrad) take k_wgrad's grid (call_plan.h: wgrad_grid), Kdot and T the Fisher call's maps.
#pragma once
#include <cstddef>
#include "fisher_tables.h"

// matrices of ld^2 doubles the call holds per entry at once: K -> L -> P, U = L^-T, Kdot, T = P Kdot (as the Fisher call)
#define HESS_MATS FISHER_MATS
// planes of the second slab: the pieces of the raw moments M3 and M4 (the gradient slab holds S, SM, SV: 3 planes)
#define HESS_HI_PLANES 2
// block sums of the W pass kept for the directions: S, SM, SV, M3, M4
#define HESS_SUMS 5

// doubles per entry of the two-plane slab of a view with the gradient slab's R x C bins
FISHER_HD inline size_t hess_hislab_stride(int Q, int R, int C) { return (size_t)HESS_HI_PLANES * Q * R * C; }
// the gradient slab has 3 planes of the same bins: a class at offset off_slab (doubles) of the gradient slab arena lies at
// off_slab / 3 * 2 of the two-plane one, and the call needs need_slab / 3 * 2 doubles of it
inline size_t hess_hislab_of(size_t gradient_slab_doubles) { return gradient_slab_doubles / 3 * HESS_HI_PLANES; }

// k_hess_beta: one workgroup per 16 rows of the class's largest entry
inline int hess_beta_grid(int nt64) { return 4 * nt64; }
// k_hess_slabsum: one thread per (plane, component, bin d >= e)
inline int hess_slabsum_grid(int Q, int D) { return (HESS_HI_PLANES * Q * (D * (D + 1) / 2) + 255) / 256; }

struct HessBuffers {
    size_t mat_doubles;      // each of Kdot and T: the plan's matrix need (every class laid out like Kmat)
    size_t coef_doubles;     // coefficient blocks of all entries (k_fisher_prep)
    size_t dir_doubles;      // each of the directions and the products on the device: nbatch * nvec * H
    size_t hislab_doubles;   // the two-plane slab of all entries
    size_t sums_doubles;     // [S | SM | SV | M3 | M4] of the W pass: HESS_SUMS * nbatch * Q D D
    size_t vec_doubles;      // [beta | diag(W)]: 2 * the plan's vector need (every class laid out like alpha)
};
inline HessBuffers hess_buffers(size_t plan_need_mat, size_t plan_need_vec, size_t plan_need_slab, int nbatch, int nvec, int H, int Q, int D) {
    const FisherBuffers fb = fisher_buffers(plan_need_mat, nbatch, nvec, H, Q, D);
    return HessBuffers{fb.mat_doubles, fb.coef_doubles, fb.dir_doubles, hess_hislab_of(plan_need_slab),
                       (size_t)HESS_SUMS * nbatch * Q * D * D, 2 * plan_need_vec};
}

// The capacity rule: the four matrices of every entry are alive at once (no memory waves), so they must fit the budget together.
inline bool hess_fits(size_t plan_need_mat, size_t mem_budget_bytes) { return fisher_fits(plan_need_mat, mem_budget_bytes); }
