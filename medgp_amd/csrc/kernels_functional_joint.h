// kernels_functional_joint.h -- the posterior covariance BETWEEN the linear functionals of a patient (medgp_functional_joint_batch).
//   ref: core/gp_regression.cpp:128-214 (predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
// The reference has no such output; the definition is tests/functional_joint_ref.py.  For two functionals f, g of one patient with the
// terms (m_k, t_k, a_k), k in f, and (m_l, t_l, a_l), l in g:
//   fcov[f, g] = q_fg - V_f^T V_g                                                          (latent: no sigma^2, no clamp)
//   q_fg = sum_{k in f} a_k sum_{l in g} a_l sum_q B_q[m_k, m_l] cos(w_q (t_k - t_l)) exp(-c_q (t_k - t_l)^2)      the prior covariance
// Works behind k_functional (kernels_functional.h) on a launch chunk of WHOLE patients: the work rows V = L^-1 K*_g of all tiles of a
// patient are resident ([npad][64] doubles per tile of 64 functionals, rows >= n zero, the columns of absent functionals zero) and so
// are its per-functional fvar.  Nothing is factored: no fp64 copy of the block is kept.
#pragma once
#include "kernels_functional.h"
#include "kernels_posterior_joint.h"   // pj_vtv, POST_KC; JointPat / JointTile: inference_tables.h

// ------------------------------------------------------------------------------------------
// One workgroup per lower 64 x 64 tile pair (I >= J) of a patient's tiles of functionals (JointPat: p0 = its first functional of the
// call, m = its functional count F, voff = its F x F block in cov).
//   acc = V_I^T V_J: k_postcov's product (pj_vtv), rows in order.
//   q_fg per element, one wave per row of the tile (row r = 4 it + w: the terms of f are the same for the whole wave and are walked
//   in a uniform loop), lane c = column: f's terms in the outer loop, g's inside, both in the caller's order, q innermost, from the
//   time DIFFERENCES in fp64 with the library's cos / exp as k_functional_prep forms q_g (no cos / sin (w t) tables: the covariance of
//   two short change scores is as small as their variances).  (sum T_I)(sum T_J) Q kernel evaluations per tile pair; the columns of a
//   wave have different term counts and lanes idle on the short ones -- the caller's order of the functionals is kept.
//   Only f > g is computed: an off-diagonal tile whole, a diagonal tile below its diagonal.  The upper triangle is mirrored from the
//   same float (cov is exactly symmetric), and the diagonal is NOT taken from the product: cov[f, f] = var[f], the float k_functional
//   rounded from its fp64 q_g - sum v^2.  A functional without terms has q = 0.0 and V = 0: its row and column are exactly 0.0f.
// An element depends on the patient, theta, the two term lists and which of the two comes first, not on the tile, the column or the
// launch chunk.  A failed entry gets NaN.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_funccov(MedgpDev L, const JointPat *__restrict__ pats, const JointTile *__restrict__ pairs, FuncTerms F,
                                                 const double *__restrict__ work, size_t work_stride, const float *__restrict__ var,
                                                 float *__restrict__ cov) {
    __shared__ double Vs[POST_KC * POST_LS];
    __shared__ double Rs[64 * POST_LS];
    __shared__ int rowk0[64], rowk1[64];
    const JointTile T = pairs[blockIdx.x];
    const JointPat P = pats[T.pat];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, g = lane >> 4;
    const int b = P.e, m = P.m, I = T.I, J = T.J;
    float *cv = cov + P.voff;
    if (L.status[b] < 0) {
        for (int x = tid; x < 64 * 64; x += 256) {
            const int i = 64 * I + (x >> 6), j = 64 * J + (x & 63);
            if (i < m && j < m) { cv[(size_t)i * m + j] = __builtin_nanf(""); cv[(size_t)j * m + i] = __builtin_nanf(""); }
        }
        return;
    }
    const int slot = L.bslot[b], n = L.pn[slot], D = L.D, Q = L.Q, npad = medgp_roundup(n, 64);
    const double *hyp = L.hyp + (size_t)b * L.hyp_stride;
    const double *B = hyp + hyp_off_B(L), *wq = hyp + hyp_off_w(L), *cq = hyp + hyp_off_c(L);
    const double *VI = work + (size_t)(P.tile0 + I) * work_stride, *VJ = work + (size_t)(P.tile0 + J) * work_stride;
    const int *toff = F.toff + P.p0;   // the term offsets of the patient's functionals
    if (tid < 64) {   // (visible after the barriers of the product)
        const bool ok = 64 * I + tid < m;
        rowk0[tid] = ok ? toff[64 * I + tid] : 0;
        rowk1[tid] = ok ? toff[64 * I + tid + 1] : 0;
    }
    const int jc = 64 * J + lane;   // this lane's column: functional jc of the patient, terms [l0, l1)
    const int l0 = jc < m ? toff[jc] : 0, l1 = jc < m ? toff[jc + 1] : 0;
    v4d acc[4];
    pj_vtv(acc, VI, VJ, npad, Vs, tid, w, li, g);
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int cs = 0; cs < 4; cs++) Rs[(16 * w + 4 * r + g) * POST_LS + 16 * cs + li] = acc[cs][r];
    __syncthreads();
#pragma unroll 1
    for (int it = 0; it < 16; it++) {
        const int r = 4 * it + w;
        if (64 * I + r >= m || jc >= m || (I == J && lane >= r)) continue;
        const int k1 = __builtin_amdgcn_readfirstlane(rowk1[r]);
        double q = 0.0;
#pragma unroll 1
        for (int k = __builtin_amdgcn_readfirstlane(rowk0[r]); k < k1; k++) {
            const double tk = F.t[k], ak = F.a[k];
            const double *Bk = B + F.m[k] * D;
            double s = 0.0;
#pragma unroll 1
            for (int l = l0; l < l1; l++) {
                const double d = tk - F.t[l], dd = d * d;
                const double *Bq = Bk + F.m[l];
                double kk = 0.0;
                for (int qi = 0; qi < Q; qi++) kk += Bq[qi * D * D] * (cos(wq[qi] * d) * exp(-cq[qi] * dd));
                s += F.a[l] * kk;
            }
            q += ak * s;
        }
        Rs[r * POST_LS + lane] = q - Rs[r * POST_LS + lane];   // (this thread's own place)
    }
    __syncthreads();
    for (int x = tid; x < 64 * 64; x += 256) {
        const int r = x >> 6, c = x & 63;
        const int i = 64 * I + r, j = 64 * J + c;
        if (i >= m || j >= m) continue;
        const float v = (I == J && c == r) ? var[P.p0 + i] : (float)((I == J && c > r) ? Rs[c * POST_LS + r] : Rs[r * POST_LS + c]);
        cv[(size_t)i * m + j] = v;
    }
    if (I != J)   // the mirrored tile, rows of cov contiguous
        for (int x = tid; x < 64 * 64; x += 256) {
            const int c = x >> 6, r = x & 63;
            const int i = 64 * I + r, j = 64 * J + c;
            if (i < m && j < m) cv[(size_t)j * m + i] = (float)Rs[r * POST_LS + c];
        }
}
