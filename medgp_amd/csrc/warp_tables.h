// warp_tables.h -- host-side geometry of medgp_warp_nlml_grad / medgp_warp_posterior_batch (kernels_warp.h): the sizes and the element
// maps of the call's own buffers, the rule that cuts k_warp_solve and the capacity rule.  Plain C++ (the element maps are also compiled
// for the device, which indexes through them): tested on the CPU by warp_tables_test.cpp under sanitizers, so a geometry mistake shows
// there and not as an out-of-bounds access on a GPU.  The posterior call's tile table and launch chunks are pjvp_tables.h's.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define WARP_HD __host__ __device__
#else
#define WARP_HD
#endif

#ifndef MEDGP_WARP_NONE   // (include/medgp_hip.h has the same two)
#define MEDGP_WARP_NONE 0
#define MEDGP_WARP_SAS  1
#endif
#define WARP_NPSI 3        // (a, eps, lambda) per covariate
#define WARP_MAX_NQ 64     // quantiles per point
// matrices of ld^2 doubles the call holds per entry at once: K -> L, U = L^-T
#define WARP_MATS 2
// vectors of ld doubles per entry: z = g(y), log g', w = L^-1 z, alpha~ = K^-1 z
#define WARP_VECS 4
enum { WARP_VEC_Z = 0, WARP_VEC_LJ = 1, WARP_VEC_W = 2, WARP_VEC_AT = 3 };

// The vector buffer holds the four roles one behind the other, each laid out like alpha (the class at off_vec, entry e of the class view
// ld further per entry): role r starts at r * plan_need_vec.
inline size_t warp_vec_offset(int role, size_t plan_need_vec) { return (size_t)role * plan_need_vec; }
WARP_HD inline size_t warp_vec_at(int e, int ld, int row) { return (size_t)e * ld + row; }

// the per-entry block of small results, indexed by the INTERNAL entry (class base k.b0 + entry of the view):
//   logjac | 1/2 |w|^2 | dpsi[D][3]
#define WARP_SMALL_HEAD 2
WARP_HD inline size_t warp_small_stride(int D) { return WARP_SMALL_HEAD + (size_t)WARP_NPSI * D; }
WARP_HD inline size_t warp_off_logjac() { return 0; }
WARP_HD inline size_t warp_off_quad() { return 1; }
WARP_HD inline size_t warp_off_dpsi(int d, int k) { return WARP_SMALL_HEAD + (size_t)WARP_NPSI * d + k; }

// the input buffer: psi of the call in the CALLER's entry order ([nbatch][D][3]), then the nq deviates
WARP_HD inline size_t warp_in_psi(int pos, int D, int d, int k) { return ((size_t)pos * D + d) * WARP_NPSI + k; }
inline size_t warp_in_zq(int nbatch, int D) { return (size_t)nbatch * D * WARP_NPSI; }

// the per-point outputs of the posterior call: zmean[M] | zvar[M] | lpd[M] | quant[M][nq]
inline size_t warp_out_zmean(size_t) { return 0; }
inline size_t warp_out_zvar(size_t M) { return M; }
inline size_t warp_out_lpd(size_t M) { return 2 * M; }
inline size_t warp_out_quant(size_t M) { return 3 * M; }
WARP_HD inline size_t warp_quant_at(size_t pt, int nq, int k) { return pt * (size_t)nq + k; }

struct WarpBuffers {
    size_t vec_doubles;     // [z | log g' | w | alpha~]: four times the plan's vector need
    size_t small_doubles;   // nbatch blocks of warp_small_stride(D)
    size_t in_doubles;      // psi [nbatch][D][3] | zq [WARP_MAX_NQ]
    size_t out_doubles;     // zmean | zvar | lpd | quant of M points (at least one point's worth)
};
inline WarpBuffers warp_buffers(size_t plan_need_vec, int nbatch, int D, size_t M, int nq) {
    const size_t Mz = M > 0 ? M : 1;
    return WarpBuffers{(size_t)WARP_VECS * plan_need_vec, (size_t)nbatch * warp_small_stride(D), (size_t)nbatch * D * WARP_NPSI + WARP_MAX_NQ,
                       (3 + (size_t)nq) * Mz};
}

// ---- the cut of k_warp_solve: ONE workgroup of four waves per entry, whatever n; both products walk the upper triangle of U in row
// order, a lane owning two adjacent columns (one 16-byte load: rows start at multiples of 64 doubles, column pairs at even columns).
//   w = U^T z      per block of WARP_SOLVE_COLS columns: wave c adds the rows j = c (mod 4), j < min(n, end of the block), in order;
//                  the four classes are added ((0 + 1) + 2) + 3
//   alpha~ = U w   row j belongs to wave j (mod 4); lane l adds the columns 2 l, 2 l + 1 of the blocks from warp_solve_first_block(j)
//                  on, in order, even column first; the 64 lane sums meet in a fixed butterfly
// Nothing here reads the launch shape: the order of every sum follows from n and the row alone.
#define WARP_SOLVE_THREADS 256
#define WARP_SOLVE_CLASSES 4
#define WARP_SOLVE_COLS 128
WARP_HD inline int warp_solve_blocks(int npad) { return (npad + WARP_SOLVE_COLS - 1) / WARP_SOLVE_COLS; }
WARP_HD inline int warp_solve_first_block(int row) { return row / WARP_SOLVE_COLS; }
// first column of the pair lane l reads in block cb; the pair is read when it lies below npad (npad is a multiple of 64: both or neither)
WARP_HD inline int warp_solve_col(int cb, int lane) { return cb * WARP_SOLVE_COLS + 2 * lane; }
// rows of U the first product reads for block cb: [0, warp_solve_rows(cb, n))
WARP_HD inline int warp_solve_rows(int cb, int n) { return (cb + 1) * WARP_SOLVE_COLS < n ? (cb + 1) * WARP_SOLVE_COLS : n; }

// The capacity rule, as the baseline calls': the two matrices of every entry are alive at once (no memory waves) beside the call's four
// vectors.  plan_need_mat / plan_need_vec: doubles of ONE matrix / vector role over all entries of the call.
inline bool warp_fits(size_t plan_need_mat, size_t plan_need_vec, size_t mem_budget_bytes) {
    const size_t lim = mem_budget_bytes / sizeof(double);
    if (plan_need_mat > lim / WARP_MATS) return false;
    const size_t mats = (size_t)WARP_MATS * plan_need_mat;
    return plan_need_vec <= (lim - mats) / (size_t)WARP_VECS;
}
