// basis_tables.h -- host-side geometry of medgp_set_basis / medgp_basis_nlml_grad / medgp_basis_posterior_batch (kernels_basis.h): the
// resident store of the bases (where a slot's rows live, when a block is reused in place, when the store is compacted into a larger
// one), the row map into the grouped order, the staging tile of k_basis_g and the k range of its triangular product.  Plain C++ (the
// element maps are also compiled for the device): tested on the CPU by basis_tables_test.cpp under sanitizers, so a geometry mistake
// shows there and not as an out-of-bounds access on a GPU.  The panels, vectors, small blocks, the capacity rule and the k range of
// the gradient pass are mean_tables.h's with p in place of D; the posterior call's tile table and launch chunks are pjvp_tables.h's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mean_tables.h"

// columns a basis carries: ONE panel of 64 columns, A = Lambda + G^T G in LDS (as MEAN_MAX_D)
#define BASIS_MAX_P MEAN_MAX_D
// k_basis_g stages BASIS_KC rows of U (64 columns of the workgroup's block) and of H (64 columns, zeros from p on) per step.  The LDS
// row stride is 16 (mod 32) doubles: the four k rows an MFMA operand read touches (lanes (li, g): row g, column li) then fall into
// the two halves of the 64 banks per 32-lane group
#define BASIS_KC 32
#define BASIS_LDS_STRIDE 80

// element (row, col) of a resident basis of p columns: rows in the GROUPED order, packed row-major
MEAN_HD inline size_t basis_h_at(int row, int p, int col) { return (size_t)row * p + col; }
// one workgroup per 64 rows of G of the class's largest entry (a workgroup beyond an entry's own blocks exits)
inline int basis_g_grid(int nt64) { return nt64; }
// the k range of block I of G = U^T H: U is upper triangular, so the rows [0, 64 (I + 1)) -- a multiple of BASIS_KC, at most npad
MEAN_HD inline int basis_g_kend(int I) { return 64 * (I + 1); }
// the last k a wave's rows 64 I + 16 w .. + 15 can meet inside the triangle (staging steps wholly beyond it carry zeros only)
MEAN_HD inline int basis_g_wave_klast(int I, int w) { return 64 * I + 16 * w + 15; }

// the failed pivot of A = Lambda + G^T G (k_basis_small): not above this times the column's own diagonal entry of A.  The pivot of a
// column that is exactly dependent on earlier ones is what rounding leaves of A_jj - sum_k L_jk^2: at most (3 + 2 p) unit roundoffs
// of A_jj, of either sign
MEAN_HD inline double basis_pivot_tol(int p) { return 4.0 * p * 2.220446049250313e-16; }

// the per-call inputs: [b0 | lam] as mean_buffers' in_doubles with p columns, and one 64-bit offset per entry (the CALLER's order)
// into the store

// ---- the resident store -------------------------------------------------------------------------------------------------------
// One device block of `cap` doubles.  A medgp_set_basis call places the rows of ALL its slots in one contiguous range, so that one
// host-to-device copy brings them: in place when the call repeats an earlier one (same slots in the same order with the same rows
// and p: the training loop's case), otherwise behind what is used.  When that does not fit, the live ranges are compacted into a new
// block (moves: device-to-device copies, in ascending source order) of at least 1.5 x the need, and the old block is retired.
// Ranges a later call replaced or a new patient dropped are dead until the next compaction.
struct BasisSlot {
    long long off = -1;   // doubles into the block; < 0: the slot has no basis
    int rows = 0, p = 0;
};
struct BasisMove { size_t src, dst, count; };
struct BasisPlace {
    size_t base = 0;       // where the call's packed rows go
    size_t new_cap = 0;    // != 0: a new block of this many doubles replaces the old one (moves first, from the old block)
    std::vector<BasisMove> moves;
};
struct BasisStore {
    size_t cap = 0, used = 0;
    std::vector<BasisSlot> slot;

    bool has(int s) const { return slot[s].off >= 0; }
    void drop(int s) { if (s >= 0 && s < (int)slot.size()) slot[s] = BasisSlot{}; }
    static size_t need(int rows, int p) { return (size_t)rows * p; }

    // nslots distinct slots with rows[k] rows of p columns each
    BasisPlace place(int nslots, const int32_t *slots, const int *rows, int p) {
        BasisPlace out;
        size_t total = 0;
        bool in_place = nslots > 0 && has(slots[0]);
        for (int k = 0; k < nslots; k++) {
            const BasisSlot &s = slot[slots[k]];
            in_place = in_place && s.off >= 0 && s.rows == rows[k] && s.p == p &&
                       (size_t)s.off == (size_t)slot[slots[0]].off + total;
            total += need(rows[k], p);
        }
        if (in_place) {
            out.base = (size_t)slot[slots[0]].off;
            return out;
        }
        for (int k = 0; k < nslots; k++) drop(slots[k]);
        if (used + total > cap) {
            // compaction: live ranges in ascending order of their offsets (ranges never overlap, so dst <= src of every move)
            std::vector<int> live;
            for (int s = 0; s < (int)slot.size(); s++)
                if (slot[s].off >= 0) live.push_back(s);
            for (size_t a = 1; a < live.size(); a++)
                for (size_t b = a; b > 0 && slot[live[b]].off < slot[live[b - 1]].off; b--) std::swap(live[b], live[b - 1]);
            size_t at = 0;
            for (int s : live) {
                const size_t cnt = need(slot[s].rows, slot[s].p);
                if (cnt) out.moves.push_back(BasisMove{(size_t)slot[s].off, at, cnt});
                slot[s].off = (long long)at;
                at += cnt;
            }
            used = at;
            const size_t want = used + total;
            out.new_cap = want > cap ? want + want / 2 : cap;
            if (out.new_cap == 0) out.new_cap = 1;
            cap = out.new_cap;
        }
        out.base = used;
        size_t at = used;
        for (int k = 0; k < nslots; k++) {
            slot[slots[k]] = BasisSlot{(long long)at, rows[k], p};
            at += need(rows[k], p);
        }
        used = at;
        return out;
    }
};

// the caller's rows packed in the grouped order: row i of the slot's range is the caller's row perm[i] (perm: internal -> caller)
inline void basis_pack_rows(const double *src, const int *perm, int rows, int p, double *dst) {
    for (int i = 0; i < rows; i++)
        for (int c = 0; c < p; c++) dst[basis_h_at(i, p, c)] = src[basis_h_at(perm[i], p, c)];
}
