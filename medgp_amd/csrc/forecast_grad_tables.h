// forecast_grad_tables.h -- the host arithmetic of medgp_forecast_grad: validation of the caller's prefix table, and the per-entry
// integer table the kernels of kernels_forecast_grad.h read.  Plain C++ on plain data (no HIP header, no kernel), like
// inference_tables.h: medgp_capi.hip includes it for the builders, the kernel header for the layout constants, and
// forecast_grad_tables_test.cpp compiles it alone with the host compiler, under sanitizers, against brute-force restatements.
//
// The table of one entry with leading dimension ld (a multiple of 64, nblk = ld / 64 blocks) is FC_TAB_INTS * ld ints:
//   [0, ld)        pfx[i]   history length p_i of observation i of the CALLER's order, FC_NONE where it is not scored (and on [n, ld))
//   [ld, 2 ld)     gpos[j]  row of the grouped order that holds the caller's observation j; the identity on [n, ld)
//   [2 ld, 3 ld)   pmin[C] (nblk) | pmax[C] (nblk) | c0 | c1 | pall | nscored:
//                  pmin / pmax: smallest / largest p_i among the scored observations of 64-block C (FC_EMPTY_MIN / -1: none);
//                  [c0, c1): the 64-blocks from the first to the last that hold a scored observation (0, 0: none);
//                  pall: the largest p_i of the entry (0: none) -- nothing behind column pall of U diag(z) is ever summed.
// The band of scored row i of L is [p_i, i]: a product over the columns of block C needs the columns k >= pmin[C] only.
#pragma once
#include <climits>
#include <cstddef>
#include <cstdint>

#define FC_TAB_INTS 3
#define FC_NONE (-1)
#define FC_EMPTY_MIN INT_MAX

// what fc_check found wrong: caller entry b, index i of the prefix table (-1: the range length), the offending value
struct FcError { int b; long long i; long long value; long long expect; };

// offsets[nbatch + 1] index prefix; entry b owns offsets[b + 1] - offsets[b] values, which must be n[b], each -1 or in [0, i].
// prefix == nullptr (everything scored, p_i = i) needs no offsets; offsets given anyway are checked.  false: *err says what is wrong.
inline bool fc_check(int nbatch, const int *n, const int64_t *offsets, const int32_t *prefix, FcError *err) {
    if (!offsets) {
        if (prefix) { *err = FcError{-1, -1, 0, 0}; return false; }
        return true;
    }
    if (offsets[0] != 0) { *err = FcError{0, -1, (long long)offsets[0], 0}; return false; }
    for (int b = 0; b < nbatch; b++) {
        const long long len = (long long)offsets[b + 1] - (long long)offsets[b];
        if (len != n[b]) { *err = FcError{b, -1, len, n[b]}; return false; }
        if (!prefix) continue;
        for (int i = 0; i < n[b]; i++) {
            const int32_t p = prefix[offsets[b] + i];
            if (p < -1 || p > i) { *err = FcError{b, (long long)offsets[b] + i, p, i}; return false; }
        }
    }
    return true;
}

// the table of one entry (layout above) into out[FC_TAB_INTS * ld].  prefix: the entry's n values, or nullptr (p_i = i);
// perm[g] = caller index of grouped row g, or nullptr (the patient was uploaded grouped: the identity).  The input has passed fc_check.
inline void fc_fill_entry(int n, int ld, const int32_t *prefix, const int *perm, int *out) {
    const int nblk = ld / 64;
    int *pfx = out, *gpos = out + ld, *blk = out + 2 * (size_t)ld;
    for (int i = 0; i < ld; i++) { pfx[i] = FC_NONE; gpos[i] = i; blk[i] = 0; }
    int *pmin = blk, *pmax = blk + nblk;
    for (int C = 0; C < nblk; C++) { pmin[C] = FC_EMPTY_MIN; pmax[C] = -1; }
    int c0 = 0, c1 = 0, pall = 0, nscored = 0;
    for (int i = 0; i < n; i++) {
        const int p = prefix ? prefix[i] : i;
        if (p < 0) continue;
        pfx[i] = p;
        const int C = i / 64;
        if (p < pmin[C]) pmin[C] = p;
        if (p > pmax[C]) pmax[C] = p;
        if (nscored == 0) c0 = C;
        c1 = C + 1;
        if (p > pall) pall = p;
        nscored++;
    }
    if (perm)
        for (int g = 0; g < n; g++) gpos[perm[g]] = g;
    // (ld = 64: nblk = 1, so the block segment holds 2 + 4 = 6 <= 64 ints; larger ld only leaves more room)
    blk[2 * nblk + 0] = c0; blk[2 * nblk + 1] = c1; blk[2 * nblk + 2] = pall; blk[2 * nblk + 3] = nscored;
}
