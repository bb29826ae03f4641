// hetero_tables.h -- host-side geometry of the heteroscedastic calls (kernels_hetero.h: medgp_set_noise_scale, medgp_hetero_nlml_grad,
// medgp_hetero_posterior_batch, medgp_robust_nlml_grad): the roles and sizes of the call's buffers, the check of a scale, the maps
// between the caller's packed rows and the grouped rows of an entry, and the capacity rule.  Plain C++ (the element maps are also
// compiled for the device): tested on the CPU by hetero_tables_test.cpp under sanitizers, so a geometry mistake shows there and not as
// an out-of-bounds access on a GPU.  The posterior call's tile table and launch chunks are pjvp_tables.h's.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__)
#define HET_HD __host__ __device__
#else
#define HET_HD
#endif

// matrices of ld^2 doubles the call holds per entry at once: K -> L, U = L^-T
#define HET_MATS 2
// vectors of ld doubles per entry: the scales s (MedgpDev::nscale), resid, fvar
#define HET_VECS 3
enum { HET_VEC_SCALE = 0, HET_VEC_RESID = 1, HET_VEC_FVAR = 2 };
// a scale lies in [2^-40, 2^40]: sigma^2 s stays a normal number beside any sigma^2 the hyper transforms produce, and 1 / s is exact
// to form
#define HET_SCALE_MIN 9.094947017729282379150390625e-13   // 2^-40
#define HET_SCALE_MAX 1099511627776.0                     // 2^40

// The vector buffer holds the three roles one behind the other, each laid out like alpha (the plan's lane base vec0, the class at
// off_vec, entry e of the class view ld further per entry): role r starts at r * het_role_stride.
inline size_t het_role_stride(size_t plan_vec0, size_t plan_need_vec) { return plan_vec0 + plan_need_vec; }
inline size_t het_vec_offset(int role, size_t role_stride) { return (size_t)role * role_stride; }
HET_HD inline size_t het_vec_at(int e, int ld, int row) { return (size_t)e * ld + row; }

inline bool het_scale_ok(double s) { return std::isfinite(s) && s >= HET_SCALE_MIN && s <= HET_SCALE_MAX; }
// index of the first scale of `count` that is not acceptable, or -1
inline int64_t het_first_bad_scale(const double *s, int64_t count) {
    for (int64_t i = 0; i < count; i++)
        if (!het_scale_ok(s[i])) return i;
    return -1;
}

// packed rows of the caller: entry b (caller's order) owns rows [off[b], off[b + 1]) with off from the entries' sizes
inline std::vector<int64_t> het_row_offsets(const int *n_of_caller_entry, int nbatch) {
    std::vector<int64_t> off((size_t)nbatch + 1, 0);
    for (int b = 0; b < nbatch; b++) off[b + 1] = off[b] + n_of_caller_entry[b];
    return off;
}
// grouped row i of a patient is the caller's row perm[i] (the stable grouping by covariate of medgp_set_patient[s]).
// caller's rows -> the grouped rows of one entry row of ld doubles; the padding rows n .. ld get 1
inline void het_rows_to_grouped(const double *src, const int *perm, int n, int ld, double *dst) {
    for (int i = 0; i < n; i++) dst[i] = src[perm[i]];
    for (int i = n; i < ld; i++) dst[i] = 1.0;
}
// the grouped rows of one entry -> the caller's rows (ok false: NaN)
inline void het_rows_to_caller(const double *src, const int *perm, int n, bool ok, double *dst) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < n; i++) dst[perm[i]] = ok ? src[i] : nan;
}

// the per-point outputs of the posterior call: mean[M] | var[M]
inline size_t het_out_mean(size_t) { return 0; }
inline size_t het_out_var(size_t M) { return M; }

struct HeteroBuffers {
    size_t vec_doubles;    // [s | resid | fvar]
    size_t out_doubles;    // mean | var of M points (at least one point's worth), then s2 of the points
    size_t tab_doubles;    // the robust call's table [nbatch][D][ROBUST_TAB] (robust_tables.h), at least one double
    size_t delta_doubles;  // per entry
};
inline HeteroBuffers hetero_buffers(size_t plan_vec0, size_t plan_need_vec, int nbatch, size_t M, size_t tab_per_entry) {
    const size_t Mz = M > 0 ? M : 1;
    return HeteroBuffers{(size_t)HET_VECS * het_role_stride(plan_vec0, plan_need_vec), 3 * Mz,
                         tab_per_entry * (size_t)nbatch > 0 ? tab_per_entry * (size_t)nbatch : 1, (size_t)nbatch};
}

// The capacity rule, as the warp calls': the two matrices of every entry are alive at once (no memory waves) beside the call's vectors.
inline bool hetero_fits(size_t plan_need_mat, size_t plan_need_vec, size_t mem_budget_bytes) {
    const size_t lim = mem_budget_bytes / sizeof(double);
    if (plan_need_mat > lim / HET_MATS) return false;
    const size_t mats = (size_t)HET_MATS * plan_need_mat;
    return plan_need_vec <= (lim - mats) / (size_t)HET_VECS;
}
