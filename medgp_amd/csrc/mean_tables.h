// mean_tables.h -- host-side geometry of medgp_mean_nlml_grad / medgp_mean_posterior_batch (kernels_mean.h): the sizes and the element
// maps of the call's own buffers, the grids of its launches and the capacity rule.  Plain C++ (the element maps are also compiled for
// the device, which indexes through them): tested on the CPU by mean_tables_test.cpp under sanitizers, so a geometry mistake shows
// there and not as an out-of-bounds access on a GPU.  The posterior call's tile table and launch chunks are pjvp_tables.h's.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define MEAN_HD __host__ __device__
#else
#define MEAN_HD
#endif

// covariates the rank-D correction carries: ONE panel of 64 columns, A = Lambda + G^T G in LDS (the entry points refuse D > 64)
#define MEAN_MAX_D 64
#define MEAN_PW 64   // doubles per panel row, whatever D (columns >= D are zero)
// matrices of ld^2 doubles the call holds per entry at once: K -> L, U = L^-T
#define MEAN_MATS 2
// panels of ld x 64 doubles per entry: G = L^-1 H, PH = K^-1 H, Pm = PH A^(-T/2)
#define MEAN_PANELS 3
// vectors of ld doubles per entry: w = L^-1 (y - H b0), alpha~
#define MEAN_VECS 2

// A panel array is laid out like alpha with 64 doubles per row: the class at 64 * off_vec, entry e of the class view ld * 64 further
// per entry.  Element (row, col) of entry e of a view of leading dimension ld:
MEAN_HD inline size_t mean_panel_at(int e, int ld, int row, int col) { return ((size_t)e * ld + row) * MEAN_PW + col; }
MEAN_HD inline size_t mean_vec_at(int e, int ld, int row) { return (size_t)e * ld + row; }

// the per-entry block of small results, indexed by the INTERNAL entry (class base k.b0 + entry of the view):
//   beta[D] | dmean[D] | delta[D] = beta - b0 | Ti[D][D] = chol(A)^-1, lower, row-major, zeros above | cov[D][D] = A^-1
MEAN_HD inline size_t mean_small_stride(int D) { return 3 * (size_t)D + 2 * (size_t)D * D; }
MEAN_HD inline size_t mean_off_beta(int) { return 0; }
MEAN_HD inline size_t mean_off_dmean(int D) { return (size_t)D; }
MEAN_HD inline size_t mean_off_delta(int D) { return 2 * (size_t)D; }
MEAN_HD inline size_t mean_off_ti(int D) { return 3 * (size_t)D; }
MEAN_HD inline size_t mean_off_cov(int D) { return 3 * (size_t)D + (size_t)D * D; }
// packed lower triangle (LDS): element (i, j), j <= i
MEAN_HD inline int mean_tri_at(int i, int j) { return i * (i + 1) / 2 + j; }

// k_mean_g and k_mean_panel: one workgroup per 64 rows of the class's largest entry (a workgroup beyond an entry's own blocks exits)
inline int mean_g_grid(int nt64) { return nt64; }
inline int mean_panel_grid(int nt64) { return nt64; }
// the k range of block I of the product PH = U G: U is upper triangular, so the columns [64 I, npad)
MEAN_HD inline int mean_panel_k0(int I) { return 64 * I; }
// the k range of the gradient pass over the Pm panel: D rounded up to the chunk of the tile product (32 columns), zeros beyond D
MEAN_HD inline int mean_wgrad_k1(int D, int kc) { return (D + kc - 1) / kc * kc; }

struct MeanBuffers {
    size_t panel_doubles;   // each of G, PH, Pm: 64 * the plan's vector need
    size_t vec_doubles;     // [w | alpha~]: twice the plan's vector need
    size_t small_doubles;   // nbatch blocks of mean_small_stride(D)
    size_t in_doubles;      // [b0 | lam], each nbatch * D, in the CALLER's entry order
};
inline MeanBuffers mean_buffers(size_t plan_need_vec, int nbatch, int D) {
    return MeanBuffers{(size_t)MEAN_PW * plan_need_vec, (size_t)MEAN_VECS * plan_need_vec, (size_t)nbatch * mean_small_stride(D), 2 * (size_t)nbatch * D};
}
// where alpha~ starts in the vector buffer, where lam starts in the input buffer
inline size_t mean_alpha_offset(size_t plan_need_vec) { return plan_need_vec; }
inline size_t mean_lam_offset(int nbatch, int D) { return (size_t)nbatch * D; }

// The capacity rule, as the Fisher call's: the two matrices and the three panels of every entry are alive at once (no memory waves), so
// they must fit the budget together.  plan_need_mat / plan_need_vec: doubles of ONE matrix / vector role over all entries of the call.
inline bool mean_fits(size_t plan_need_mat, size_t plan_need_vec, size_t mem_budget_bytes) {
    const size_t lim = mem_budget_bytes / sizeof(double);
    if (plan_need_mat > lim / MEAN_MATS) return false;
    const size_t mats = (size_t)MEAN_MATS * plan_need_mat;
    return plan_need_vec <= (lim - mats) / ((size_t)MEAN_PANELS * MEAN_PW);
}
