// medgp_capi.hip -- C ABI of libmedgp_hip.so (see include/medgp_hip.h) and the launch pipeline.
// gfx950 only; there is deliberately no CPU fallback: without a HIP device every compute entry
// point fails with MEDGP_ERR_NODEVICE.
#include "../../include/medgp_hip.h"
#include "medgp_dev.h"
#include "call_plan.h"
#include "kernels_core.h"
#include "kernels_v0.h"
#include "kernels_cholinv.h"
#include "kernels_cholinv_la.h"
#include "kernels_assemble.h"
#include "kernels_wgrad.h"
#include "kernels_io.h"
#include "kernels_cohort.h"
#include "kernels_gmm.h"
#include "kernels_posterior.h"
#include "kernels_posterior_joint.h"
#include "kernels_forecast.h"
#include "kernels_trend.h"
#include "kernels_components.h"
#include "kernels_functional.h"
#include "kernels_functional_joint.h"
#include "kernels_loo.h"
#include "kernels_loo_grad.h"
#include "kernels_forecast_grad.h"
#include "kernels_lgo_grad.h"
#include "kernels_fisher.h"
#include "kernels_hess.h"
#include "kernels_posterior_jvp.h"
#include "kernels_posterior_vjp.h"
#include "kernels_mean.h"
#include "kernels_basis.h"
#include "kernels_warp.h"
#include "kernels_hetero.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

namespace {

enum KernelId { KID_PREP = 0, KID_ASSEMBLE, KID_CHOLINV, KID_LA_STEP, KID_LA_AUX, KID_LAUUM, KID_GRADBINS, KID_WGRAD, KID_EPILOGUE, KID_PREDICT, KID_ALPHA, KID_POSTERIOR, KID_POSTCOV, KID_POSTFACTOR, KID_POSTDRAW, KID_LOO_DIAG, KID_LOO_GRAM, KID_LOO_SOLVE, KID_LOO_KINV, KID_LOO_VEC, KID_LOO_WGRAD, KID_TREND, KID_FORECAST, KID_FC_VEC, KID_FC_T, KID_FC_SCAN, KID_FC_QM, KID_FC_TABLES, KID_FC_WGRAD, KID_LGO_VEC, KID_LGO_INV, KID_LGO_S, KID_LGO_T, KID_LGO_WGRAD, KID_FI_PREP, KID_FI_KDOT, KID_FI_T, KID_FI_WGRAD, KID_HE_MOMENTS, KID_HE_SLABSUM, KID_HE_BETA, KID_HE_WGRAD, KID_HE_EPILOGUE, KID_PJ_SOLVE, KID_PJ_U, KID_PJ_DIR, KID_PV_COT, KID_PV_WGRAD, KID_PV_CROSS, KID_PV_FINISH, KID_MN_G, KID_MN_SMALL, KID_MN_PANEL, KID_MN_WGRAD, KID_MN_POST, KID_BS_G, KID_BS_SMALL, KID_BS_POST, KID_WP_Z, KID_WP_SOLVE, KID_WP_SMALL, KID_WP_POST, KID_HT_LOAD, KID_HT_ROWS, KID_HT_ESTEP, KID_HT_OBJ, KID_HT_POST, KID_COUNT };
constexpr int KID_EXT_COUNT = KID_BS_POST + 1;   // what medgp_profile_num_kernels_ext is pinned at; [KID_EXT_COUNT, KID_EXT2_COUNT): the _ext2 entries
constexpr int KID_EXT2_COUNT = KID_WP_POST + 1;  // what medgp_profile_num_kernels_ext2 is pinned at; [KID_EXT2_COUNT, KID_COUNT): the _ext3 entries
const char *const kKernelNames[KID_COUNT] = {"k_prep", "k_assemble", "k_cholinv", "k_la_step", "k_la_aux", "k_lauum", "k_gradbins", "k_wgrad", "k_epilogue", "k_predict", "k_alpha", "k_posterior", "k_postcov", "k_postfactor", "k_postdraw", "k_loo_diag", "k_loo_gram", "k_loo_solve", "k_loo_kinv", "k_loo_vec", "k_loo_wgrad", "k_trend", "k_forecast", "k_fc_vec", "k_fc_t", "k_fc_scan", "k_fc_qm", "k_fc_tables", "k_fc_wgrad", "k_lgo_vec", "k_lgo_inv", "k_lgo_s", "k_lgo_t", "k_lgo_wgrad", "k_fisher_prep", "k_fisher_kdot", "k_fisher_t", "k_fisher_wgrad", "k_hess_moments", "k_hess_slabsum", "k_hess_beta", "k_hess_wgrad", "k_hess_epilogue", "k_pjvp_solve", "k_pjvp_u", "k_pjvp_dir", "k_pvjp_cot", "k_pvjp_wgrad", "k_pvjp_cross", "k_pvjp_finish", "k_mean_g", "k_mean_small", "k_mean_panel", "k_mean_wgrad", "k_mean_post", "k_basis_g", "k_basis_small", "k_basis_post", "k_warp_z", "k_warp_solve", "k_warp_small", "k_warp_post", "k_het_load", "k_het_rows", "k_het_estep", "k_het_obj", "k_het_post"};

thread_local std::string g_create_error;   // last medgp_create error of the calling thread

struct EvPair { int kid; hipEvent_t a, b; };

constexpr int kAuxStreams = 4;

// ---- device memory arenas (round 6) -----------------------------------------------------------------------------------------
// The per-entry buffers of a context live in ARENAS: one hipMalloc block each, sized ONCE where the caller can say what it will need
// (medgp_reserve for capacities below 8 GB of matrices -- every BASELINE configuration; medgp_reserve_plan from the patients' sizes)
// and otherwise replaced by a larger block when a call outgrows it.  What round 6 measured about memory on this platform
// (scratch/alloc_cost.hip, alloc_dirty.hip, vmm_repro.hip, vmm_stress.hip -> profiles/r06_memory_findings.txt; MI355X, ROCm 7.2):
//   * hipMalloc / hipFree cost microseconds on a fresh device (48 GB: 0.3 ms), but memory that has been USED and freed -- by this or
//     an earlier process -- is wiped by the driver, and an allocation that is handed such memory waits for the wipe: 24 GB after
//     another process had freed 250 GB took 6.5 s, a 100 GB block 2-3 s on its second use inside one process.  Rounds 1-5 grew the
//     arenas by hipDeviceSynchronize + hipFree + hipMalloc(1.5 x) and sized screening chunks at 26 + 9 GB: BENCH_r05's 9.5 s of
//     screening on the driver's box against 5.1 s on the builder's was this.  The cure is to obtain LITTLE memory, ONCE: nlml-only
//     plans have no Linv (half the bytes), screening chunks hold 2 GB instead of 48, the trainer announces its sizes before its loop.
//   * Virtual-memory management (hipMemAddressReserve / hipMemCreate / hipMemMap / hipMemSetAccess: grow in place, never free, never
//     move) was built first and REMOVED: on this runtime hipMemSetAccess on the second chunk of a range fails with "invalid argument"
//     for some size / address patterns (24 MB then 2 MB; 2 MB then 24 MB with alignment 0), a reservation is booked against the
//     device's free-memory counter as if it were memory (one 256 GB reservation: "Free memory set to zero", every later call fails),
//     and re-mapping chunks into a larger range left stale translations behind -- a later range read another arena's data
//     (vmm_stress: mismatches in every arena after the first).  Plain blocks it is.
//   * A growth waits for NOTHING: the outgrown block is retired (queued kernels may still read it) and freed at the context's next idle
//     point (round 5: hipDeviceSynchronize + hipFree first -- every other context sharing the GPU stalled); it asks for 1.5 x and
//     retries with exactly what is needed if that fails.
struct Arena {
    char *base = nullptr;
    size_t bytes = 0;    // size of the block
};
// The device buffers of the inference entry points (medgp_fit_predict*, medgp_posterior*_batch, medgp_forecast_batch, medgp_loo_*): own
// blocks, replaced when a call outgrows them (buf_ensure), freed by free_all.  The calls block and run in stream order, so buffers of
// one role are shared between them:
//   per-point inputs / outputs of the call, the tile table, the work rows of one launch chunk (at most posterior_budget bytes unless
//   one tile needs more; medgp_fit_predict*: the k* rows) -- BUF_T2, BUF_META2, BUF_MEAN, BUF_VAR, BUF_TILES and BUF_WORK, which every
//   call that takes test points (or the terms of functionals) fills in ONE step, upload_point_call, reads through launch_pjvp_solve /
//   for_solved_chunks where it starts from V = L^-1 K*, and brings home through download_pair (unsort_pair where the device's point
//   order is not the caller's); the forecast's prefix and y2; lpd (forecast: per point, LOO: per group);
//   joint posterior: the patient / tile-pair / row-block tables of the call, C and the float covariance blocks of one launch chunk, the
//   call's eps and samples, cov_status -- LOO: its group / tile-pair / job tables, the blocks of one launch chunk, group_status;
//   LOO: the singleton table and the index lists; BUF_GVEC: the per-entry vectors [u | s | v | log p] of medgp_loo_grad;
//   BUF_SLOPE: the per-point outputs [dmean | dvar | cross] of medgp_trend_batch;
//   BUF_COMP: the per-point outputs [cmean | cvar | ccov] of medgp_components_batch (Q, Q and Q^2 floats per point);
//   medgp_functional_batch (T terms, F functionals; the terms' covariates and times travel as the posterior call's points, the outputs
//   in its mean / var): BUF_FUNC_D the doubles [weight T | rsum T | q_g F | cos T Q | sin T Q], BUF_FUNC_I the ints [toff F + 1 | fun T];
//   medgp_functional_joint_batch: besides, the joint posterior's patient and tile-pair tables and its float covariance blocks (fcov)
//   medgp_forecast_grad: BUF_GVEC holds its per-entry vectors [g / 2 | e | lpd | -], BUF_FC_TAB the per-entry integer tables
//   (forecast_grad_tables.h), BUF_FC_T the matrix T = U Mbar of every entry, laid out like Kmat (gradient calls only)
//   medgp_lgo_grad: BUF_GVEC holds its per-entry vectors [r | s | v | log p] (k_loo_vec's layout), the LOO call's group / tile-pair /
//   job tables, index lists, blocks (BUF_C), lpd and group_status buffers; BUF_LGO_COLS / _TROWS / _SGL / _ENT / _GORD the tables of
//   build_lgo_tables; BUF_LGO_T the matrix Tt = P S of every entry, laid out like Kmat (gradient calls only)
//   medgp_fisher_vec (fisher_tables.h): BUF_FI_KDOT / BUF_FI_T the matrices Kdot and T = P Kdot of every entry for the direction in
//   hand, laid out like Kmat; BUF_FI_COEF the direction's coefficient blocks; BUF_FI_DIR the caller's directions [nbatch][nvec][H];
//   BUF_FI_OUT the products, direction-major [nvec][nbatch][H] (k_epilogue's row stride is H)
//   medgp_hess_vec (hess_tables.h): the five Fisher buffers in the same roles; BUF_HE_SLAB the two-plane slab of the raw moments M3, M4;
//   BUF_HE_SUMS the block sums [S | SM | SV | M3 | M4] of the W pass, each [nbatch][Q D D]; BUF_HE_VEC [beta | diag(W)], each laid out
//   like alpha
//   medgp_posterior_jvp_batch (pjvp_tables.h): BUF_FI_KDOT, BUF_FI_COEF, BUF_FI_DIR in the Fisher call's roles; BUF_PJ_U u = Kdot alpha,
//   laid out like alpha; BUF_PJ_OUT [dmean | dvar], each [M][nvec]; the per-point buffers, the tile table and the work rows in the
//   posterior call's roles
//   medgp_posterior_vjp_batch (pvjp_tables.h): BUF_PV_ENT the per-entry records, BUF_PV_SEG the covariate ranges of every entry's
//   points, BUF_PV_ORD caller point -> device point; BUF_PV_IN the caller's per-point inputs, BUF_PV_PTS the cotangents, loss terms and
//   cos / sin tables of the points, BUF_PV_VEC c = W cm (laid out like alpha), BUF_PV_SMALL per entry [sum cv D | loss | -], BUF_PV_OUT
//   the gradients, set-major [ncot][nbatch][H]; the per-point buffers, the tile table and the work rows in the posterior call's roles
//   medgp_mean_nlml_grad / medgp_mean_posterior_batch (mean_tables.h): BUF_MN_G, BUF_MN_PH, BUF_MN_PM the panels G = L^-1 H, K^-1 H and
//   Pm (laid out like alpha, 64 doubles per row), BUF_MN_VEC [w | alpha~], BUF_MN_SMALL the per-entry blocks (beta^, dmean, delta,
//   chol(A)^-1, A^-1), BUF_MN_IN [b0 | lam] in the caller's order, BUF_MN_OUT the fp64 [mean | var] of the posterior call's points
//   medgp_basis_nlml_grad / medgp_basis_posterior_batch (basis_tables.h): the seven buffers above in the same roles with p columns;
//   BUF_BS_OFF the offset of every entry's rows in the resident store (caller's order), BUF_BS_H2 the basis rows of the call's points
//   medgp_warp_nlml_grad / medgp_warp_posterior_batch (warp_tables.h): BUF_WP_VEC [z | log g' | w | alpha~], each laid out like alpha,
//   BUF_WP_SMALL the per-entry blocks (logjac, 1/2 |w|^2, dpsi), BUF_WP_IN [psi | zq] (psi in the caller's order), BUF_WP_KIND kind[D],
//   BUF_WP_Y2 the observed values at the call's points, BUF_WP_OUT the fp64 [zmean | zvar | lpd | quant] of the posterior call's points
//   medgp_hetero_nlml_grad / medgp_hetero_posterior_batch / medgp_robust_nlml_grad (hetero_tables.h): BUF_HT_VEC [s | resid | fvar], each
//   laid out like alpha (s is what MedgpDev::nscale points at during the call), BUF_HT_OUT the fp64 [mean | var | s2] of the posterior
//   call's points, BUF_HT_TAB the robust call's table (robust_tables.h, the caller's order), BUF_HT_DELTA its per-entry delta,
//   BUF_HT_HAS per internal entry whether its slot has resident scales
struct DevBuf { void *p = nullptr; size_t cap = 0; };   // cap: bytes
enum BufId { BUF_T2 = 0, BUF_META2, BUF_MEAN, BUF_VAR, BUF_PARTS, BUF_TILES, BUF_WORK, BUF_PREFIX, BUF_Y2, BUF_LPD,
             BUF_PATS, BUF_PAIRS, BUF_BLKS, BUF_C, BUF_COV, BUF_EPS, BUF_SAMP, BUF_CSTAT, BUF_SINGLES, BUF_ROWS, BUF_GVEC, BUF_SLOPE, BUF_COMP, BUF_FUNC_D, BUF_FUNC_I, BUF_FC_T, BUF_FC_TAB, BUF_LGO_T, BUF_LGO_COLS, BUF_LGO_TROWS, BUF_LGO_SGL, BUF_LGO_ENT, BUF_LGO_GORD, BUF_FI_KDOT, BUF_FI_T, BUF_FI_COEF, BUF_FI_DIR, BUF_FI_OUT, BUF_HE_SLAB, BUF_HE_SUMS, BUF_HE_VEC, BUF_PJ_U, BUF_PJ_OUT, BUF_PV_ENT, BUF_PV_SEG, BUF_PV_ORD, BUF_PV_IN, BUF_PV_PTS, BUF_PV_VEC, BUF_PV_SMALL, BUF_PV_OUT, BUF_MN_G, BUF_MN_PH, BUF_MN_PM, BUF_MN_VEC, BUF_MN_SMALL, BUF_MN_IN, BUF_MN_OUT, BUF_BS_OFF, BUF_BS_H2, BUF_WP_VEC, BUF_WP_SMALL, BUF_WP_IN, BUF_WP_KIND, BUF_WP_Y2, BUF_WP_OUT, BUF_HT_VEC, BUF_HT_OUT, BUF_HT_TAB, BUF_HT_DELTA, BUF_HT_HAS, BUF_COUNT };
constexpr size_t kArenaEager = (size_t)8 << 30;
enum ArenaId { AR_K = 0, AR_U, AR_Z, AR_ALPHA, AR_WDIAG, AR_CS, AR_SN, AR_SLAB, AR_LA_PART, AR_LA_SMALL, AR_COUNT };

}  // namespace

struct medgp_ctx {
    int device = -1;
    int kidx = 0, R = 0, H = 0, nlik = 0;
    PlanRules rules;          // what the plan of a call reads of the context (call_plan.h): Q, D, num_cu, max_batch, the budgets and the route knobs
    double pi = 3.14159265;   // ref: util/global_settings.h:6
    hipStream_t own_stream = nullptr, stream = nullptr;
    int max_slots = 0, max_n = 0, ldn = 0;
    MedgpDev dev{};
    // device allocations
    std::vector<void *> allocs;
    int *d_proff = nullptr, *d_pcoff = nullptr, *d_jit = nullptr, *d_bn = nullptr;
    int *d_pn = nullptr, *d_pmeta = nullptr, *d_pseg = nullptr, *d_bslot = nullptr, *d_status = nullptr;
    double *d_pt = nullptr, *d_py = nullptr;
    MedgpPrior *d_prior = nullptr;
    uint8_t *d_prior_on = nullptr;
    double *d_theta = nullptr, *d_nlml = nullptr, *d_grad = nullptr;   // staging for the host-pointer API (= lane 0)
    int *d_status_out = nullptr;
    // second lane of the asynchronous host-pointer API (medgp_nlml_grad_async): lane 0 uses the buffers above
    double *d_theta1 = nullptr, *d_nlml1 = nullptr, *d_grad1 = nullptr;
    int *d_status1 = nullptr;
    hipEvent_t ev_lane[2] = {nullptr, nullptr};
    // copy streams of the asynchronous lanes: the theta upload of one lane and the result download of the other run beside the
    // kernels on c->stream (on the compute stream they were 9 MB of PCIe traffic per 512-patient step, serialised with the kernels)
    hipStream_t s_up = nullptr, s_down = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_k[2] = {nullptr, nullptr};
    bool lane_pending[2] = {false, false};
    // pinned staging ring for small host-to-device uploads (slot tables, prior descriptors): the source of an asynchronous
    // copy must stay untouched until the copy has run, and nothing here waits for the device on the normal path
    char *pin_buf[2] = {nullptr, nullptr};
    size_t pin_cap = 0, pin_off = 0;
    int pin_cur = 0;
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_pending[2] = {false, false};
    char *h_small = nullptr;               // pinned landing area of the host-pointer operator's results (small calls)
    char *d_small = nullptr;               // ... and their device image [nlml | grad | status]: ONE copy brings a small call's results back
    MedgpPrior *d_prior_stage = nullptr;   // device staging of medgp_set_prior[s] rows
    int *d_prior_slots = nullptr;
    size_t prior_stage_rows = 0;
    // host mirrors
    std::vector<int> h_n;
    std::vector<std::vector<int>> h_perm;   // internal index -> caller index
    std::vector<uint8_t> h_perm_identity;
    std::vector<int> h_bslot;       // effective slots of the last call, CALLER order
    int last_nbatch = 0;
    BatchPlan plan;                 // of the last call
    // arenas of the per-entry buffers (Kmat, Linv, z, alpha, wdiag, cs, sn, slab, look-ahead scratch): what medgp_reserve's capacities
    // would need at most (full_*).  Up to kArenaEager bytes they are allocated by medgp_reserve; beyond
    // that (a ragged cohort whose largest patient is far above the median: max_batch x max_n^2 would not fit 288 GB) they grow with the
    // calls or are sized once by medgp_reserve_plan (struct Arena).
    size_t full_mat = 0, full_vec = 0, full_tab = 0, full_slab = 0;
    Arena arena[AR_COUNT];
    // blocks that outgrown arenas left behind: kernels queued before the growth may still read them, so they are NOT freed there (no
    // wait at the growth) but at the next point where the context's streams are known to be idle (free_retired)
    std::vector<void *> retired;
    size_t retired_bytes = 0;
    double alloc_s = 0.0;           // wall seconds inside device / pinned memory management calls (medgp_alloc_stats)
    long long alloc_calls = 0;
    int *d_bpos = nullptr;
    int *d_tpos = nullptr;          // theta rows of the entries (medgp_screen), internal order
    bool tpos_on = false;
    double *d_screen_theta = nullptr;   // the block of hyper vectors of medgp_screen
    size_t screen_theta_cap = 0;
    bool last_has_inverse = false;   // the last pipeline run formed alpha and U = L^-T (medgp_get_factor is valid)
    // upload staging (one pinned host buffer + one device buffer, reused; guarded by ev_stage)
    char *h_stage = nullptr, *d_stage = nullptr;
    size_t stage_cap = 0;
    hipEvent_t ev_stage = nullptr;
    bool stage_pending = false;
    // scratch of the look-ahead multi-CU factorisation (kernels_cholinv_la.h), grown on demand
    // (arena[AR_LA_PART], arena[AR_LA_SMALL])
    char *h_bounce = nullptr;        // pinned bounce buffer for the large device-to-host exports (factor matrices)
    size_t bounce_cap = 0;
    int *d_one_slot = nullptr;       // single-entry slot table for the caller-order re-factorisation of medgp_get_factor
    DevBuf buf[BUF_COUNT];          // the inference entry points' buffers (enum BufId)
    // the resident bases of medgp_set_basis (basis_tables.h): ONE device block, the host's map of it, and the pinned buffer the packed
    // rows of a call travel through (guarded by ev_basis)
    BasisStore basis;
    double *d_basis = nullptr;
    char *h_basis_stage = nullptr;
    size_t basis_stage_cap = 0;
    hipEvent_t ev_basis = nullptr;
    bool basis_pending = false;
    // the resident noise scales of medgp_set_noise_scale (kernels_hetero.h): [max_slots][ldn] in the grouped row order, allocated by the
    // first call that sets any; h_has_scale: which slots hold some (a new patient in a slot drops them)
    double *d_slot_scale = nullptr;
    std::vector<uint8_t> h_has_scale;
    std::vector<int64_t> pv_src;    // medgp_posterior_vjp_batch: device point -> caller point of the last call (medgp_posterior_vjp_moments)
    bool pv_valid = false;          // ... and whether BUF_PV_PTS still holds that call's fp64 mean / var
    size_t posterior_budget = (size_t)2 << 30;   // MEDGP_POSTERIOR_BUDGET_GB
    // profiling
    bool profiling = false;
    int profile_only = -1;    // >= 0: only launches of this kernel id are bracketed (medgp_profile_enable(ctx, 2 + id))
    int wgrad_deep = -1;      // MEDGP_WGRAD_DEEP=1/2: force the prefetch depth of k_wgrad's operand stream (A-B; same bits); -1: by launch size
    int la_park = 256;        // MEDGP_LA_PARK=<workgroup id>|0: where the look-ahead schedule parks its sleeping workgroup (0 = off)
    int la_park_maxbatch = 8; // MEDGP_LA_PARK_MAXBATCH: largest batch the parking is used for (measured: 4 x N=2048 -5 %, 16 x N=2048 +2 %)
    int dbg_fail = 0;         // MEDGP_DEBUG_FAIL_ATTEMPTS=k: test hook, see MedgpDev::dbg_fail
    int class_streams = kAuxStreams;   // MEDGP_CLASS_STREAMS=0: the size classes of a call run back to back on the call's stream (A-B)
    hipStream_t aux[kAuxStreams] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kAuxStreams] = {nullptr, nullptr, nullptr, nullptr};
    // second lane of medgp_screen (round 6): chunks alternate between c->stream and s_screen1, each with its own rows of the batch
    // buffers and its own half of the arenas -- the assembly of one chunk runs beside the factorisation of the other
    hipStream_t s_screen1 = nullptr;
    hipEvent_t ev_fork1 = nullptr, ev_screen0 = nullptr;
    char *h_screen_tab = nullptr;   // pinned: the slot / position / theta-row tables of ALL chunks of one medgp_screen call
    size_t screen_tab_cap = 0;
    std::vector<EvPair> events;
    std::vector<hipEvent_t> ev_pool;   // recycled timing events: a profiled launch creates none once the pool is warm
    double prof_ms[KID_COUNT] = {0};
    int64_t prof_n[KID_COUNT] = {0};
    std::string err;
};

namespace {

int fail(medgp_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(c, call)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return fail((c), MEDGP_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
int dalloc(medgp_ctx *c, T **p, size_t count) {
    void *q = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
    c->alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->alloc_calls++;
    if (e != hipSuccess) return fail(c, MEDGP_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", count * sizeof(T), hipGetErrorString(e));
    c->allocs.push_back(q);
    *p = (T *)q;
    return MEDGP_OK;
}

void arena_release(medgp_ctx *c, Arena &A);
void free_all(medgp_ctx *c) {
    for (void *p : c->allocs) (void)hipFree(p);
    c->allocs.clear();
    for (int i = 0; i < AR_COUNT; i++) arena_release(c, c->arena[i]);
    for (void *p : c->retired) (void)hipFree(p);
    c->retired.clear();
    c->retired_bytes = 0;
    for (DevBuf &b : c->buf) {
        if (b.p) (void)hipFree(b.p);
        b = DevBuf{};
    }
}

template <typename T>
T *buf(medgp_ctx *c, int id) { return (T *)c->buf[id].p; }

// at least `bytes` in buffer `id`: the block is kept when large enough, otherwise replaced after the queued work that may still read it
int buf_ensure(medgp_ctx *c, int id, size_t bytes) {
    DevBuf &b = c->buf[id];
    if (bytes <= b.cap && b.p) return MEDGP_OK;
    const auto t0 = std::chrono::steady_clock::now();
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(b.p);
        b = DevBuf{};
    }
    const size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&b.p, want);
    c->alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    c->alloc_calls++;
    if (e != hipSuccess) { b.p = nullptr; return fail(c, MEDGP_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e)); }
    b.cap = want;
    return MEDGP_OK;
}

// Dispatch on the component count Q: f is a generic lambda called with std::integral_constants, so that every launch site names its
// kernel template once.  with_q8: <Q> for 1 .. 8, else <0> (the kernel's generic component loop).
template <int N> using QConst = std::integral_constant<int, N>;
template <class F>
void with_q8(int Q, F &&f) {
    switch (Q) {
    case 1: f(QConst<1>{}); break;
    case 2: f(QConst<2>{}); break;
    case 3: f(QConst<3>{}); break;
    case 4: f(QConst<4>{}); break;
    case 5: f(QConst<5>{}); break;
    case 6: f(QConst<6>{}); break;
    case 7: f(QConst<7>{}); break;
    case 8: f(QConst<8>{}); break;
    default: f(QConst<0>{}); break;
    }
}
// with_q16: f(<Q>, <0>) for 1 .. 8; for 9 .. 16 f(<8>, <0>), then f(<Q - 8>, <8>) for the rest of the components; false (nothing called)
// for any other Q: the caller takes its generic route
template <class F>
bool with_q16(int Q, F &&f) {
    if (Q < 1 || Q > 16) return false;
    if (Q > 8) f(QConst<8>{}, QConst<0>{});
    with_q8(Q > 8 ? Q - 8 : Q, [&](auto q) {
        if constexpr (decltype(q)::value > 0) { if (Q > 8) f(q, QConst<8>{}); else f(q, QConst<0>{}); }
    });
    return true;
}

int num_cov(int kidx, int Q, int D, int R) {
    switch (kidx) {
    case MEDGP_KERNEL_LMC_SM: return Q * (D * R + 2 + D);
    case MEDGP_KERNEL_SM: return 3 * Q;
    case MEDGP_KERNEL_SE: return 2;
    default: return -1;
    }
}

struct Launcher {
    medgp_ctx *c;
    int kid;
    hipStream_t st;
    hipEvent_t a = nullptr, b = nullptr;
    bool on;
    Launcher(medgp_ctx *c_, int kid_, hipStream_t st_ = nullptr) : c(c_), kid(kid_), st(st_ ? st_ : c_->stream) {
        on = c->profiling && (c->profile_only < 0 || c->profile_only == kid);
        if (on) {
            a = take(); b = take();
            (void)hipEventRecord(a, st);
        }
    }
    hipEvent_t take() {
        hipEvent_t e = nullptr;
        if (!c->ev_pool.empty()) { e = c->ev_pool.back(); c->ev_pool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    }
    void finish() {   // closes the bracket now (the destructor then does nothing)
        if (on) {
            (void)hipEventRecord(b, st);
            if (kid >= 0) c->events.push_back({kid, a, b});
            else { c->ev_pool.push_back(a); c->ev_pool.push_back(b); }   // recorded but never read: safe to re-record later
            on = false;
        }
    }
    ~Launcher() { finish(); }
};

// ---- the tail of every gradient: block sums of the slab, then the gradient lines (kernels_core.h) -- on the stream the caller runs on
// the block sums S, SM, SV of the nb entries of the view V from the slab its tile kernel filled
void launch_slabsum(medgp_ctx *c, hipStream_t stream, const MedgpDev &V, int nb) {
    const int nbins3 = 3 * V.Q * tri(V.D);
    Launcher l(c, KID_EPILOGUE, stream);
    hipLaunchKernelGGL(k_slabsum, dim3(nb, (nbins3 + 255) / 256), dim3(256), 0, stream, V);
}
// the gradient lines (flag_grad; from_slab: from the block sums) and the scalar `mode` names, into the caller's rows of nlml / grad / status
void launch_epilogue(medgp_ctx *c, hipStream_t stream, const MedgpDev &V, int nb, const double *theta, int flag_grad, int from_slab,
                     double *nlml, double *grad, int *status, EpilogueMode mode) {
    const dim3 grid(nb, epilogue_parts(nb, c->rules.num_cu, V.H, MEDGP_EPI_PARTS));
    Launcher l(c, KID_EPILOGUE, stream);
    hipLaunchKernelGGL(k_epilogue, grid, dim3(256), 0, stream, V, theta, flag_grad, from_slab, nlml, grad, status, (int)mode);
}
// The tail of a size class of a call whose objective an earlier kernel left in scal[2] (LOO, LGO, forecast score, baseline nlml): for
// a gradient the block sums, then the epilogue into the context's result staging.
void finish_objective_class(medgp_ctx *c, const MedgpDev &V, int nb, int flag_grad) {
    if (flag_grad) launch_slabsum(c, c->stream, V, nb);
    launch_epilogue(c, c->stream, V, nb, c->d_theta, flag_grad, 1, c->d_nlml, c->d_grad, c->d_status_out, EPI_OBJECTIVE);
}
// One launch (two for 9 .. 16 components, each on its own components: kernels_wgrad.h) of a kernel that walks the tiles of
// wgrad_grid, under label kid: f(q, q0, grid, block) names the kernel.  Every caller has refused Q > 16.
template <class F>
void launch_tiles(medgp_ctx *c, int kid, int Q, const WgradGrid &wg, F &&f) {
    Launcher l(c, kid);
    with_q16(Q, [&](auto q, auto q0) { f(q, q0, dim3(wg.grid), dim3(WG_THREADS)); });
}
// k_wgrad over the tiles of wg for the nb entries of the view V (kernels_wgrad.h), under the caller's Launcher: two launches for 9 .. 16
// components, each reducing its own components into its own slab planes.  The one home of the prefetch-depth rule: few large patients
// (the launch fills the chip less than four times) prefetch their operands two chunks ahead and walk the tiles in serpentine order.
// False: Q > 16, nothing was launched (the nlml gradient then takes its generic route).
bool launch_wgrad(medgp_ctx *c, hipStream_t stream, const MedgpDev &V, int nb, const WgradGrid &wg) {
    const int pf = c->wgrad_deep >= 0 ? c->wgrad_deep : ((long)nb * wg.wg_tiles <= 16L * c->rules.num_cu ? 2 : 1);
    const dim3 tg(wg.grid), tb(WG_THREADS);
    return with_q16(V.Q, [&](auto q, auto q0) {
        constexpr int QQ = decltype(q)::value, Q0 = decltype(q0)::value;
        if (pf >= 2) hipLaunchKernelGGL((k_wgrad<QQ, Q0, 2>), tg, tb, 0, stream, V, nb, wg.wg_tiles, wg.nbp);
        else hipLaunchKernelGGL((k_wgrad<QQ, Q0, 1>), tg, tb, 0, stream, V, nb, wg.wg_tiles, wg.nbp);
    });
}

int drain_events(medgp_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &e : c->events) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            c->prof_ms[e.kid] += ms;
            c->prof_n[e.kid] += 1;
        }
        c->ev_pool.push_back(e.a);
        c->ev_pool.push_back(e.b);
    }
    c->events.clear();
    return MEDGP_OK;
}

// A pinned region of `bytes` that stays untouched until every copy queued from it on c->stream so far has run.  Two buffers:
// when one is full its event is recorded and the other one is taken (waiting only if THAT buffer's copies from a whole
// ring revolution ago are still in flight, which in practice never happens).
int pin_stage(medgp_ctx *c, size_t bytes, void **out) {
    bytes = (bytes + 63) & ~(size_t)63;
    if (bytes > c->pin_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < 2; i++) { if (c->pin_buf[i]) (void)hipHostFree(c->pin_buf[i]); c->pin_buf[i] = nullptr; c->pin_pending[i] = false; }
        const size_t cap = std::max<size_t>(2 * bytes, (size_t)1 << 20);
        for (int i = 0; i < 2; i++) HIPCHK(c, hipHostMalloc((void **)&c->pin_buf[i], cap, hipHostMallocDefault));
        c->pin_cap = cap; c->pin_off = 0; c->pin_cur = 0;
    }
    for (int i = 0; i < 2; i++) if (!c->pin_ev[i]) HIPCHK(c, hipEventCreateWithFlags(&c->pin_ev[i], hipEventDisableTiming));
    if (c->pin_off + bytes > c->pin_cap) {
        HIPCHK(c, hipEventRecord(c->pin_ev[c->pin_cur], c->stream));
        c->pin_pending[c->pin_cur] = true;
        c->pin_cur ^= 1;
        if (c->pin_pending[c->pin_cur]) { HIPCHK(c, hipEventSynchronize(c->pin_ev[c->pin_cur])); c->pin_pending[c->pin_cur] = false; }
        c->pin_off = 0;
    }
    *out = c->pin_buf[c->pin_cur] + c->pin_off;
    c->pin_off += bytes;
    return MEDGP_OK;
}

// Select the batch and lay out its plan.  caller_order: entries whose patient was not uploaded grouped by output use the caller-order
// copy of the patient (slot + max_slots), so that the factor is the one the caller's order defines (no gradient on that copy).
int set_batch(medgp_ctx *c, int nbatch, const int32_t *slots, bool caller_order, bool with_u) {
    if (nbatch < 1 || nbatch > c->rules.max_batch) return fail(c, MEDGP_ERR_CAPACITY, "nbatch %d outside [1, %d]", nbatch, c->rules.max_batch);
    std::vector<int> eff(nbatch), en(nbatch);
    for (int b = 0; b < nbatch; b++) {
        int s = slots[b];
        if (s < 0 || s >= c->max_slots || c->h_n[s] < 0) return fail(c, MEDGP_ERR_ARG, "slots[%d] = %d is not a resident patient", b, s);
        en[b] = c->h_n[s];
        eff[b] = (caller_order && !c->h_perm_identity[s]) ? s + c->max_slots : s;
    }
    bool same = (nbatch == c->last_nbatch) && c->plan.with_u == with_u && std::memcmp(c->h_bslot.data(), eff.data(), sizeof(int) * nbatch) == 0;
    if (same) return MEDGP_OK;
    std::memcpy(c->h_bslot.data(), eff.data(), sizeof(int) * nbatch);
    BatchPlan &P = c->plan;
    layout_plan(c->rules, en.data(), nbatch, with_u, P);
    // the tables travel through the pinned ring: no wait for the device (the lock-step optimiser changes the active set on
    // most steps; stream order puts the copy behind the kernels of the previous call that still read the old tables)
    const bool need_pos = !(P.identity && P.cls.size() == 1);
    void *pin = nullptr;
    int rcp = pin_stage(c, sizeof(int) * nbatch * (need_pos ? 2 : 1), &pin);
    if (rcp) return rcp;
    int *hp = (int *)pin;
    for (int i = 0; i < nbatch; i++) hp[i] = eff[P.order[i]];
    HIPCHK(c, hipMemcpyAsync(c->d_bslot, hp, sizeof(int) * nbatch, hipMemcpyHostToDevice, c->stream));
    if (need_pos) {
        for (int i = 0; i < nbatch; i++) hp[nbatch + i] = P.order[i];
        HIPCHK(c, hipMemcpyAsync(c->d_bpos, hp + nbatch, sizeof(int) * nbatch, hipMemcpyHostToDevice, c->stream));
    }
    c->last_nbatch = nbatch;
    return MEDGP_OK;
}

// the view of the batch buffers one size class works in (entry 0 of the view = internal entry k.b0)
MedgpDev class_view(const medgp_ctx *c, const BatchPlan &P, const SizeClass &k) {
    const MedgpDev &L = c->dev;
    MedgpDev V = L;
    const size_t Q = L.Q, D = L.D, b0 = (size_t)k.b0 + (size_t)P.row0;
    V.ldn = k.ld;
    const SlabGeom sg = slab_geom(k.ld, L.Q, L.D);
    V.slab_R = sg.R; V.slab_C = sg.C; V.slab_stride = sg.stride;
    V.bslot = L.bslot + b0;
    V.bpos = (P.identity && P.cls.size() == 1) ? nullptr : c->d_bpos + b0;
    V.tpos = c->tpos_on ? c->d_tpos + b0 : nullptr;
    V.hyp = L.hyp + b0 * L.hyp_stride;
    V.cs = L.cs + P.tab0 + k.off_tab; V.sn = L.sn + P.tab0 + k.off_tab;
    V.Kmat = L.Kmat + P.mat0 + k.off_mat; V.Linv = L.Linv + (P.with_u ? P.mat0 + k.off_mat : 0);
    V.z = L.z + P.vec0 + k.off_vec; V.alpha = L.alpha + P.vec0 + k.off_vec; V.wdiag = L.wdiag + P.vec0 + k.off_vec;
    if (L.nscale) V.nscale = L.nscale + P.vec0 + k.off_vec;   // (a heteroscedastic call is running: HeteroScope)
    V.epi_lp = L.epi_lp + b0 * MEDGP_EPI_PARTS; V.epi_ticket = L.epi_ticket + b0;
    V.scal = L.scal + b0 * 4; V.status = L.status + b0; V.jit = L.jit + b0; V.bn = L.bn + b0; V.xk = L.xk + b0 * 64 * 64;
    V.S = L.S + b0 * Q * D * D; V.SM = L.SM + b0 * Q * D * D; V.SV = L.SV + b0 * Q * D * D;
    V.slab = L.slab + k.off_slab;
    return V;
}

// view of the batch-indexed buffers starting at entry b0 of the view L
MedgpDev shifted_view(const MedgpDev &L, int b0) {
    MedgpDev V = L;
    const size_t ld = L.ldn, Q = L.Q, D = L.D;
    V.bslot = L.bslot + b0;
    if (L.bpos) V.bpos = L.bpos + b0;
    if (L.tpos) V.tpos = L.tpos + b0;
    V.hyp = L.hyp + (size_t)b0 * L.hyp_stride;
    V.cs = L.cs + (size_t)b0 * Q * ld; V.sn = L.sn + (size_t)b0 * Q * ld;
    V.Kmat = L.Kmat + (size_t)b0 * ld * ld; V.Linv = L.Linv + (size_t)b0 * ld * ld;
    V.z = L.z + (size_t)b0 * ld; V.alpha = L.alpha + (size_t)b0 * ld; V.wdiag = L.wdiag + (size_t)b0 * ld;
    if (L.nscale) V.nscale = L.nscale + (size_t)b0 * ld;
    V.epi_lp = L.epi_lp + (size_t)b0 * MEDGP_EPI_PARTS; V.epi_ticket = L.epi_ticket + b0;
    V.scal = L.scal + (size_t)b0 * 4; V.status = L.status + b0; V.jit = L.jit + b0; V.bn = L.bn + b0; V.xk = L.xk + (size_t)b0 * 64 * 64;
    V.S = L.S + (size_t)b0 * Q * D * D; V.SM = L.SM + (size_t)b0 * Q * D * D; V.SV = L.SV + (size_t)b0 * Q * D * D;
    V.slab = L.slab + (size_t)b0 * L.slab_stride;
    return V;
}

// the one-entry view of CALLER entry b of the last call
MedgpDev entry_view(const medgp_ctx *c, int b) {
    const int i = c->plan.inv[b];
    for (const SizeClass &k : c->plan.cls)
        if (i >= k.b0 && i < k.b0 + k.count) return shifted_view(class_view(c, c->plan, k), i - k.b0);
    return c->dev;   // (not reached: every entry belongs to a class)
}

// device -> host copy of `bytes` through a pinned bounce buffer (a pageable hipMemcpy of this size pays ~10 ms of one-time
// runtime staging set-up on its first use); returns the pinned pointer, valid until the next call
int d2h_pinned(medgp_ctx *c, const void *dev, size_t bytes, const char **out) {
    if (bytes > c->bounce_cap) {
        if (c->h_bounce) (void)hipHostFree(c->h_bounce);
        c->h_bounce = nullptr; c->bounce_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->h_bounce, bytes + bytes / 4, hipHostMallocDefault));
        c->bounce_cap = bytes + bytes / 4;
    }
    HIPCHK(c, hipMemcpyAsync(c->h_bounce, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = c->h_bounce;
    return MEDGP_OK;
}

// ---- arenas: one block each, sized once where possible, replaced (never waited for) where not (see struct Arena) ----------------
struct AllocTimer {   // wall time of the memory-management calls, for medgp_alloc_stats
    medgp_ctx *c;
    std::chrono::steady_clock::time_point t0;
    explicit AllocTimer(medgp_ctx *c_) : c(c_), t0(std::chrono::steady_clock::now()) {}
    ~AllocTimer() { c->alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); c->alloc_calls++; }
};

void arena_release(medgp_ctx *c, Arena &A) {
    AllocTimer tm(c);
    if (A.base) (void)hipFree(A.base);
    A = Arena{};
}

// every stream of the context is idle afterwards (NOT the device: other contexts / ranks that share it keep running)
int sync_ctx_streams(medgp_ctx *c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < kAuxStreams; i++) if (c->aux[i]) HIPCHK(c, hipStreamSynchronize(c->aux[i]));
    if (c->s_up) HIPCHK(c, hipStreamSynchronize(c->s_up));
    if (c->s_down) HIPCHK(c, hipStreamSynchronize(c->s_down));
    if (c->s_screen1) HIPCHK(c, hipStreamSynchronize(c->s_screen1));
    return MEDGP_OK;
}

// the blocks outgrown arenas left behind; the caller guarantees that every stream of the context is idle
void free_retired(medgp_ctx *c, bool timed = true) {
    if (c->retired.empty()) return;
    const auto t0 = std::chrono::steady_clock::now();
    for (void *p : c->retired) (void)hipFree(p);
    if (timed) { c->alloc_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); c->alloc_calls++; }
    c->retired.clear();
    c->retired_bytes = 0;
}

// make at least `bytes` of arena `id` usable.  exact: the caller knows this is the high-water mark (medgp_reserve, medgp_reserve_plan):
// allocate just that; otherwise 1.5 x what was there (at most `limit` bytes, the most the capacities of medgp_reserve allow), with a
// retry at exactly `bytes`.  *moved is set when the block was replaced: its contents are gone.
// The old block is RETIRED, not freed: kernels queued earlier may still read it, and neither they nor anything else is waited for here
// (round 5 synchronised the whole device and freed first).  Retired blocks are freed at the next idle point of the context (the end of a
// blocking call, medgp_synchronize), at once when they add up to more than half the memory budget, or when the device is out of memory.
int arena_ensure(medgp_ctx *c, int id, size_t bytes, size_t limit, bool exact, bool *moved) {
    Arena &A = c->arena[id];
    if (bytes <= A.bytes) return MEDGP_OK;
    AllocTimer tm(c);
    const size_t old = A.bytes;
    if (A.base) { c->retired.push_back(A.base); c->retired_bytes += A.bytes; }
    A = Arena{};
    if (c->retired_bytes > c->rules.mem_budget / 2) { int rc = sync_ctx_streams(c); if (rc) return rc; free_retired(c, false); }
    size_t want = exact ? bytes : std::max(bytes, old + old / 2);
    if (limit >= bytes) want = std::min(want, limit);
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, want);
    if (e != hipSuccess && !c->retired.empty()) {   // out of memory with retired blocks around: give them back first
        (void)hipGetLastError();
        int rc = sync_ctx_streams(c); if (rc) return rc;
        free_retired(c, false);
        e = hipMalloc(&q, want);
    }
    if (e != hipSuccess && want > bytes) { (void)hipGetLastError(); want = bytes; e = hipMalloc(&q, want); }   // near capacity the 1.5 x request can fail where `bytes` fits
    if (e != hipSuccess) return fail(c, MEDGP_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
    A.base = (char *)q; A.bytes = want;
    if (moved) *moved = true;
    return MEDGP_OK;
}

// the arenas of the per-entry buffers of the batch views: doubles needed of Kmat, Linv (0: an nlml-only plan never touches it),
// z / alpha / wdiag, cs / sn, slab.  exact: see arena_ensure.
int ensure_arena(medgp_ctx *c, size_t need_k, size_t need_u, size_t need_vec, size_t need_tab, size_t need_slab, bool exact = false) {
    MedgpDev &L = c->dev;
    bool moved = false, mv;
    int rc;
    auto one = [&](int id, size_t need, size_t full, double **p) -> int {
        mv = false;
        if ((rc = arena_ensure(c, id, std::max<size_t>(need, 8) * sizeof(double), full * sizeof(double), exact, &mv))) return rc;
        *p = (double *)c->arena[id].base;
        moved = moved || mv;
        return MEDGP_OK;
    };
    if ((rc = one(AR_K, need_k, c->full_mat, &L.Kmat))) return rc;
    if ((rc = one(AR_U, need_u, c->full_mat, &L.Linv))) return rc;
    if ((rc = one(AR_Z, need_vec, c->full_vec, &L.z))) return rc;
    if ((rc = one(AR_ALPHA, need_vec, c->full_vec, &L.alpha))) return rc;
    if ((rc = one(AR_WDIAG, need_vec, c->full_vec, &L.wdiag))) return rc;
    if ((rc = one(AR_CS, need_tab, c->full_tab, &L.cs))) return rc;
    if ((rc = one(AR_SN, need_tab, c->full_tab, &L.sn))) return rc;
    if ((rc = one(AR_SLAB, need_slab, c->full_slab, &L.slab))) return rc;
    if (moved) c->last_has_inverse = false;   // (the factors of earlier calls are gone)
    return MEDGP_OK;
}

// scratch of the look-ahead factorisation for the classes of a wave that take it: two arenas, carved up per class (la_layout,
// call_plan.h) -- the classes run on different streams.  args[i] = the kernel arguments of v[i]; part0 / small0: the lane base of the
// plan (doubles).
int ensure_la(medgp_ctx *c, const std::vector<LaNeed> &v, bool with_u, std::vector<LaArgs> &args, size_t part0 = 0, size_t small0 = 0) {
    size_t need_part = part0, need_small = small0;
    for (const LaNeed &e : v) { const LaLayout Y = la_layout(e, with_u); need_part += Y.part_doubles; need_small += Y.small_doubles; }
    int rc;
    // (a block that must grow is replaced; the old one is retired, not freed: kernels queued on any of the context's streams may still read it)
    if ((rc = arena_ensure(c, AR_LA_PART, need_part * sizeof(double), 0, false, nullptr))) return rc;
    if ((rc = arena_ensure(c, AR_LA_SMALL, need_small * sizeof(double), 0, false, nullptr))) return rc;
    double *pp = (double *)c->arena[AR_LA_PART].base + part0, *ps = (double *)c->arena[AR_LA_SMALL].base + small0;
    args.clear();
    for (const LaNeed &e : v) {
        const LaLayout Y = la_layout(e, with_u);
        LaArgs A{};
        A.nbmax = e.nbmax; A.maxslice = Y.maxslice; A.rows = Y.rows;
        A.ring = 1;
        A.nbatch = e.count;
        A.part = pp;
        A.ybuf = ps + Y.ybuf; A.xk2 = ps + Y.xk2; A.pnx = ps + Y.pnx; A.pnx2 = ps + Y.pnx2;
        A.dterm = ps + Y.dterm; A.dsum = ps + Y.dsum; A.dpart = ps + Y.dpart;
        A.flag = (int *)(ps + Y.flag);
        args.push_back(A);
        pp += Y.part_doubles; ps += Y.small_doubles;
    }
    return MEDGP_OK;
}

// one kernel chain for the `nbatch` entries of the view L (a size class of the call) on `stream`; nt64 = 64-blocks of its largest entry,
// entry_n = their sizes (host mirror), route = how they are factored, la = the look-ahead scratch (ROUTE_LA only)
int run_pipeline_one(medgp_ctx *c, hipStream_t stream, const MedgpDev &L, int nbatch, int nt64, const double *theta_dev,
                     int flag_grad, bool need_inverse, int min_n, double *nlml_dev, double *grad_dev, int32_t *status_dev,
                     bool store_ukk, const int *entry_n, int route, const LaArgs *la_in) {
    const WgradGrid wg = wgrad_grid(entry_n, nbatch, nt64);
    const bool ragged = wg.ragged;
    { Launcher l(c, KID_PREP, stream); hipLaunchKernelGGL(k_prep, dim3(nbatch, 1 + (L.Q * L.ldn + PREP_CHUNK - 1) / PREP_CHUNK + ((theta_dev && L.kidx == 7) ? (L.Q * L.D * L.D + PREP_BCHUNK - 1) / PREP_BCHUNK : 0)), dim3(256), 0, stream, L, theta_dev, min_n); }
    auto launch_assemble = [&]() {
        Launcher l(c, KID_ASSEMBLE, stream);
        const dim3 tg(tri(nt64), nbatch), tb(256);
        // 9 .. 16 components: the first eight, then the rest added to the same tiles (kernels_assemble.h)
        // (a heteroscedastic call -- L.nscale set, Q <= 16, never the generic route -- takes the instantiation that scales the noise: the
        //  noise is added by the pass that starts at component 0)
        if (L.nscale) {
            with_q16(L.Q, [&](auto q, auto q0) {
                constexpr int QQ = decltype(q)::value, Q0 = decltype(q0)::value;
                hipLaunchKernelGGL((k_assemble_t<QQ, Q0, Q0 == 0>), tg, tb, 0, stream, L);
            });
            return;
        }
        if (c->rules.use_v0 || !with_q16(L.Q, [&](auto q, auto q0) { hipLaunchKernelGGL((k_assemble_t<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, stream, L); }))
            hipLaunchKernelGGL(k_assemble_v0, tg, tb, 0, stream, L);   // Q > 16 (or MEDGP_V0): generic kernel
    };
    const bool inv = flag_grad || need_inverse;
    const int want_mode = inv ? 1 : (store_ukk ? 2 : 0);   // bit 0: U rows + alpha; 2: diagonal blocks U_kk only (k_predict)
    // Few large patients: the multi-CU look-ahead schedule (kernels_cholinv_la.h) instead of one workgroup per patient; which classes
    // of a call take it is decided by choose_routes (call_plan.h: the route rule).
    const bool multi_cu = route == ROUTE_LA;
    if (multi_cu) {
        // which entries the multi-CU schedule factors: more than one 64-block (host mirror of the patient sizes)
        bool any_small = false;
        for (int bb = 0; bb < nbatch; bb++) any_small = any_small || entry_n[bb] <= 64;
        {
            const LaArgs la = *la_in;
            launch_assemble();
            // entries of a single 64-block: one workgroup each (the same kernel, hence the same bits, as in any other call)
            if (any_small) { Launcher l(c, KID_CHOLINV, stream); hipLaunchKernelGGL((k_cholinv<8, 4, 1>), dim3(nbatch), dim3(512), 0, stream, L, want_mode); }
            const int nbx = ragged ? (nbatch | 1) : nbatch;   // x extent of the look-ahead grids: odd for a ragged class (LaArgs::nbatch)
            { Launcher l(c, KID_LA_AUX, stream); hipLaunchKernelGGL(k_la_prologue, dim3(nbx, 1 + nt64), dim3(LA_THREADS), 0, stream, L, la, want_mode); }
            auto step_counts = [&](int k, int *nF, int *nLrows, int *nsl) {
                const int nMF = std::max(nt64 - (k + 2), 0), nUF = (want_mode & 1) ? k + 1 : 0, nUL = (want_mode & 1) ? k : 0;
                *nF = nMF + nUF + 1;
                *nLrows = (k + 2 < nt64 && k >= 1) ? nMF + nUL + 1 : 0;
                *nsl = std::min(la.maxslice, (k + la_slice_len(k) - 1) / la_slice_len(k));   // history slices that exist at step k
            };
            // look-ahead schedule: one launch per 64-wide step (kernels_cholinv_la.h)
            for (int k = 0; k < nt64; k++) {
                int nF, nLrows, nsl;
                step_counts(k, &nF, &nLrows, &nsl);
                // single entry: park a sleeping workgroup where the dispatcher would put the chain's first neighbour (kernels_cholinv_la.h)
                const int ntask = 1 + LA_NAUX(k) + nF + nLrows * nsl;   // D, the F row blocks, R and / or H, the look-ahead slices
                // (workgroup ids are y * nbatch + x: with nbatch entries the chains are ids 0 .. nbatch-1 and their first neighbours
                //  ids 256 .. 256+nbatch-1, i.e. task y = 256 / nbatch of every entry)
                const int pk = (c->la_park > 0 && nbx == nbatch && nbatch <= c->la_park_maxbatch && c->la_park % nbatch == 0) ? c->la_park / nbatch : -1;
                const int park = (pk > 0 && ntask > pk && k + 1 < nt64) ? pk : -1;
                Launcher l(c, KID_LA_STEP, stream);
                hipLaunchKernelGGL(k_la_step, dim3(nbx, ntask + (park >= 0 ? 1 : 0)), dim3(LA_THREADS), 0, stream, L, la, k, want_mode, nLrows, park);
            }
            { Launcher l(c, KID_LA_AUX, stream); hipLaunchKernelGGL(k_la_finish, dim3(nbx, 4 * nt64), dim3(256), 0, stream, L, la, want_mode); }
            // The reference's retry loop (c_inference_exact.cpp:99-111: add the noise vector again, at most 10 times), device
            // driven: entries whose one attempt above failed (status -2) are re-assembled and factored by k_cholinv's in-kernel
            // loop; for healthy entries this launch is one workgroup that reads a status word.  No host read-back, no wait.
            { Launcher l(c, KID_CHOLINV, stream); hipLaunchKernelGGL((k_cholinv<8, 4, 2>), dim3(nbatch), dim3(512), 0, stream, L, want_mode); }
        }
    } else {
        launch_assemble();
        Launcher l(c, KID_CHOLINV, stream);
        // more patients than CUs: 4-wave workgroups, two per CU (the serial diagonal phase of one overlaps the MFMA phase of the
        // other).  At most one patient per CU: 8 waves (8 block slots per pass) once a step has more than 4 row blocks, else the
        // 4-wave shape, whose 4 slots already cover every block of n <= 256 (measured, 256 patients x N=256, D=2: <4,4> 0.211 ms,
        // <8,4> 0.232 ms -- half of its 8 slots idle).
        // Only shapes with at most two waves per SIMD are instantiated: the out-of-line diagonal factor (diag_factor_wave) is
        // compiled ONCE for the tightest register budget among its callers -- with a <*,2> shape (four waves per SIMD, 128 VGPRs)
        // in the library it is held to 128 VGPRs and carries 182 scratch accesses on the serial path of EVERY shape (248 VGPRs and
        // 18 without; found when the legacy k_ci_panel caller that had masked this left the build: k_cholinv<4,4> 1.37 -> 1.48 ms).
#ifdef MEDGP_PRICE_NLML
        // pricing build (results meaningless): MEDGP_PRICE_SHAPE=43 / 42 runs the nlml-only calls in a shape with 3 / 4 workgroups per CU
        static const int price_shape = getenv("MEDGP_PRICE_SHAPE") ? atoi(getenv("MEDGP_PRICE_SHAPE")) : 0;
        if (want_mode == 0 && route == ROUTE_WG44 && price_shape == 43) hipLaunchKernelGGL((k_cholinv<4, 3, 0>), dim3(nbatch), dim3(256), 0, stream, L, want_mode);
        else if (want_mode == 0 && route == ROUTE_WG44 && price_shape == 42) hipLaunchKernelGGL((k_cholinv<4, 2, 0>), dim3(nbatch), dim3(256), 0, stream, L, want_mode);
        else
#endif
        if (route == ROUTE_WG44) hipLaunchKernelGGL((k_cholinv<4, 4, 0>), dim3(nbatch), dim3(256), 0, stream, L, want_mode);
        else hipLaunchKernelGGL((k_cholinv<8, 4, 0>), dim3(nbatch), dim3(512), 0, stream, L, want_mode);
    }
    int from_slab = 0;
#ifdef MEDGP_STAMPS
    if (getenv("MEDGP_DBG_NOWGRAD")) { HIPCHK(c, hipGetLastError()); return MEDGP_OK; }
#endif
    if (flag_grad) {
        Launcher lw(c, KID_WGRAD, stream);
        from_slab = !c->rules.use_v0 && launch_wgrad(c, stream, L, nbatch, wg);   // Q > 16 (or MEDGP_V0): generic kernels below
        if (!from_slab) lw.kid = -1;   // nothing was launched under this label: its events go back to the pool unread
        lw.finish();
        if (!from_slab) {
            { Launcher l(c, KID_LAUUM, stream); hipLaunchKernelGGL(k_lauum_v0, dim3(tri(nt64), nbatch), dim3(256), 0, stream, L); }
            const int nbins = L.Q * tri(L.D);
            { Launcher l(c, KID_GRADBINS, stream); hipLaunchKernelGGL(k_gradbins_v0, dim3((nbins + 255) / 256, nbatch), dim3(256), 0, stream, L); }
        }
    }
    if (flag_grad && from_slab) launch_slabsum(c, stream, L, nbatch);
    if (nlml_dev) launch_epilogue(c, stream, L, nbatch, theta_dev, flag_grad, from_slab, nlml_dev, grad_dev, (int *)status_dev, EPI_NLML);
    HIPCHK(c, hipGetLastError());
    return MEDGP_OK;
}


// The evaluation pipeline; everything is asynchronous and ordered on c->stream.  Every size class of the plan gets its own kernel
// chain; with more than one class the chains run on auxiliary streams forked from / joined into c->stream, so that the workgroup-per-
// patient launches of the small classes fill the CUs a look-ahead chain of the large ones leaves idle.  The plan it carries out --
// classes, waves, offsets, routes, look-ahead scratch -- is call_plan.h's (layout_plan in set_batch, plan_needs here).
// persist: the caller reads per-entry buffers of ALL entries after the call (factor exports, k_predict): such a call must fit one wave.
// Pp / st_main / aux0, naux: the plan to run, the stream its first class runs on and the auxiliary streams its other classes may use --
// the context's own (c->plan, c->stream, all of c->aux) unless medgp_screen runs two plans at once on two lanes.
int run_pipeline(medgp_ctx *c, const double *theta_dev, int flag_grad, bool need_inverse, int min_n,
                 double *nlml_dev, double *grad_dev, int32_t *status_dev, bool store_ukk = false, bool persist = false,
                 BatchPlan *Pp = nullptr, hipStream_t st_main = nullptr, int aux0 = 0, int naux = kAuxStreams, hipEvent_t ev_fork_in = nullptr) {
    BatchPlan &P = Pp ? *Pp : c->plan;
    if (!st_main) st_main = c->stream;
    hipEvent_t ev_fork = ev_fork_in ? ev_fork_in : c->ev_fork;
    const bool forms_u = flag_grad || need_inverse || store_ukk;
    if (forms_u && !P.with_u) return fail(c, MEDGP_ERR_ARG, "internal: plan laid out without Linv for a call that forms it");
    if (persist && P.nwaves > 1)
        return fail(c, MEDGP_ERR_CAPACITY, "the call's per-entry matrices exceed the memory budget of %zu GB (MEDGP_MEM_BUDGET_GB) and its outputs need all of them at once: split the call",
                    c->rules.mem_budget >> 30);
    std::vector<LaNeed> las;
    std::vector<int> la_of;
    const PlanNeeds nd = plan_needs(c->rules, P, las, la_of);   // (chooses the routes of the classes; the look-ahead arenas grow wave by wave below)
    { int rc = ensure_arena(c, P.mat0 + nd.mat, P.with_u ? P.mat0 + nd.mat : 0, P.vec0 + nd.vec, P.tab0 + nd.tab, nd.slab); if (rc) return rc; }
    c->last_has_inverse = (flag_grad || need_inverse) && P.nwaves == 1;
    const int nstr = std::max(0, std::min(c->class_streams, naux));
    for (int w = 0; w < P.nwaves; w++) {
        // this wave's classes [i0, i1) and their look-ahead scratch
        size_t i0 = 0, i1;
        while (i0 < P.cls.size() && P.cls[i0].wave != w) i0++;
        i1 = i0;
        while (i1 < P.cls.size() && P.cls[i1].wave == w) i1++;
        std::vector<LaNeed> wl;
        std::vector<int> wl_of(P.cls.size(), -1);
        for (size_t i = i0; i < i1; i++) if (la_of[i] >= 0) { wl_of[i] = (int)wl.size(); wl.push_back(las[la_of[i]]); }
        std::vector<LaArgs> wa;
        if (!wl.empty()) { int rc = ensure_la(c, wl, P.with_u, wa, P.la_part0, P.la_small0); if (rc) return rc; }
        const bool fork = i1 - i0 > 1 && nstr > 0 && c->aux[aux0];
        if (fork) HIPCHK(c, hipEventRecord(ev_fork, st_main));
        bool used[kAuxStreams] = {false, false, false, false};
        for (size_t i = i0; i < i1; i++) {
            const SizeClass &k = P.cls[i];
            hipStream_t st = st_main;
            int ai = -1;
            if (fork && i > i0) {   // the wave's first class (its largest entries) stays on the call's stream
                ai = aux0 + (int)((i - i0 - 1) % nstr);
                st = c->aux[ai];
                if (!used[ai]) { HIPCHK(c, hipStreamWaitEvent(st, ev_fork, 0)); used[ai] = true; }
            }
            const MedgpDev V = class_view(c, P, k);
            int rc = run_pipeline_one(c, st, V, k.count, k.nbmax, theta_dev, flag_grad, need_inverse, min_n, nlml_dev, grad_dev, status_dev, store_ukk,
                                      P.en.data() + k.b0, k.route, wl_of[i] >= 0 ? &wa[wl_of[i]] : nullptr);
            if (rc) return rc;
        }
        if (fork)
            for (int ai = aux0; ai < aux0 + nstr; ai++)
                if (used[ai]) {
                    HIPCHK(c, hipEventRecord(c->ev_join[ai], c->aux[ai]));
                    HIPCHK(c, hipStreamWaitEvent(st_main, c->ev_join[ai], 0));
                }
    }
    return MEDGP_OK;
}

// ---- what the inference entry points share (fit_predict, factor, posterior, joint posterior, forecast, LOO, LOO gradient) ------
// the context is reserved, the batch fits it and every slot holds a patient
int check_call(medgp_ctx *c, int nbatch, const int32_t *slots) {
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (nbatch < 1 || nbatch > c->rules.max_batch) return fail(c, MEDGP_ERR_CAPACITY, "nbatch %d outside [1, %d]", nbatch, c->rules.max_batch);
    for (int b = 0; b < nbatch; b++)
        if (slots[b] < 0 || slots[b] >= c->max_slots || c->h_n[slots[b]] < 0) return fail(c, MEDGP_ERR_ARG, "slots[%d] = %d is not a resident patient", b, slots[b]);
    return MEDGP_OK;
}

// ---- what every call that takes test points shares: check_points, stage_points, upload_point_call, launch_pjvp_solve /
// ---- for_solved_chunks (the calls that start from V = L^-1 K*), download_pair / unsort_pair; call_plan.h: scatter_entry_blocks ------
// the covariates of n points (or terms) lie in [0, D); SE / SM read none
int check_meta2(medgp_ctx *c, int64_t n, const int32_t *meta2) {
    if (!meta2 || c->kidx != MEDGP_KERNEL_LMC_SM) return MEDGP_OK;
    for (int64_t j = 0; j < n; j++)
        if (meta2[j] < 0 || meta2[j] >= c->rules.D) return fail(c, MEDGP_ERR_ARG, "meta2[%lld] = %d outside [0, %d)", (long long)j, meta2[j], c->rules.D);
    return MEDGP_OK;
}

// The test points of a call: patient b owns points [offsets[b], offsets[b + 1]) of meta2 / t2 and of the call's per-point arrays.
// Returns their number M, or the (negative) error code.  missing: one of the per-point arrays the call REQUIRES is null, `outs` names
// them for the message; outs null: the call's per-point outputs are optional and t2 alone is named.
int64_t check_points(medgp_ctx *c, int nbatch, const int64_t *offsets, const int32_t *meta2, const float *t2, bool missing, const char *outs) {
    if (offsets[0] != 0) return fail(c, MEDGP_ERR_ARG, "offsets[0] = %lld, expected 0", (long long)offsets[0]);
    for (int b = 0; b < nbatch; b++)
        if (offsets[b + 1] < offsets[b]) return fail(c, MEDGP_ERR_ARG, "offsets decrease at %d", b);
    const int64_t M = offsets[nbatch];
    if (M > (int64_t)INT32_MAX - POST_TW) return fail(c, MEDGP_ERR_ARG, "%lld test points in one call (at most %d)", (long long)M, INT32_MAX - POST_TW);
    if (M > 0 && (!t2 || missing)) return outs ? fail(c, MEDGP_ERR_ARG, "t2 / %s is NULL", outs) : fail(c, MEDGP_ERR_ARG, "t2 is NULL");
    if (M > 0 && c->kidx == MEDGP_KERNEL_LMC_SM && !meta2) return fail(c, MEDGP_ERR_ARG, "meta2 is NULL for the multi-output kernel");
    const int rc = check_meta2(c, M, meta2);
    return rc ? rc : M;
}

// the M checked test points as the device takes them (double times, int outputs): device point k is the caller's point src[k] (null: k)
void stage_points(medgp_ctx *c, int64_t M, const int32_t *meta2, const float *t2, const int64_t *src, std::vector<double> &ht2, std::vector<int> &hm2) {
    ht2.resize(M);
    hm2.assign(M, 0);
    const bool lmc = meta2 && c->kidx == MEDGP_KERNEL_LMC_SM;
    for (int64_t k = 0; k < M; k++) {
        const int64_t j = src ? src[k] : k;
        ht2[k] = (double)t2[j];
        if (lmc) hm2[k] = meta2[j];
    }
}

// theta to the device and the ONE pipeline run of an inference call: factor and z = L^-1 y of every entry, with U = L^-T and
// alpha = K^-1 y (need_inverse: medgp_get_factor is valid afterwards) or the diagonal-block inverses U_kk (store_ukk).  The call reads
// per-entry buffers of all entries afterwards: it must fit one memory wave.  min_n: entries of fewer observations get status -1 (k_prep).
int factor_run(medgp_ctx *c, int nbatch, const double *theta, bool need_inverse, bool store_ukk, int min_n = 1) {
    HIPCHK(c, hipMemcpyAsync(c->d_theta, theta, sizeof(double) * c->H * nbatch, hipMemcpyHostToDevice, c->stream));
    return run_pipeline(c, c->d_theta, 0, need_inverse, min_n, nullptr, nullptr, nullptr, store_ukk, true);
}

// The end of a blocking call: the status words of its entries are read back behind whatever the caller has queued, the stream is
// waited for, and they are scattered from the plan's internal order to the caller's (status; null: not wanted).  internal: the words
// in internal order, for callers that go on with them.
int read_status(medgp_ctx *c, int nbatch, int32_t *status, std::vector<int> *internal = nullptr) {
    std::vector<int> tmp;
    std::vector<int> &st = internal ? *internal : tmp;
    st.assign(nbatch, 0);
    if (status || internal) HIPCHK(c, hipMemcpyAsync(st.data(), c->d_status, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (status) for (int i = 0; i < nbatch; i++) status[c->plan.order[i]] = st[i];
    return MEDGP_OK;
}

// the size classes of the last plan as the table builders take them (inference_tables.h)
std::vector<TableClass> table_classes(const BatchPlan &P) {
    std::vector<TableClass> v;
    for (const SizeClass &k : P.cls) v.push_back({k.b0, k.count, k.ld});
    return v;
}
// host table -> buffer `id` (grown as needed); an empty table uploads nothing
template <class T>
int upload_table(medgp_ctx *c, int id, const std::vector<T> &v) {
    if (v.empty()) return MEDGP_OK;
    int rc = buf_ensure(c, id, v.size() * sizeof(T));
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->buf[id].p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return MEDGP_OK;
}

// The upload step of a call of M points: the per-point buffers (BUF_T2, BUF_META2, BUF_MEAN, BUF_VAR) and the staged points on their
// way into them, the tile table into BUF_TILES and work_need bytes of work rows in BUF_WORK.  A call without tiles still gets a
// BUF_WORK block (buf_ensure's 256-byte minimum: the kernels of medgp_posterior_vjp_batch take the pointer even then); for the other
// calls that is one small allocation on a context that never had points, nothing on any later call.
template <class Tile>
int upload_point_call(medgp_ctx *c, int64_t M, const std::vector<double> &ht2, const std::vector<int> &hm2, const std::vector<Tile> &tiles,
                      size_t work_need) {
    const size_t Mz = (size_t)std::max<int64_t>(M, 1);
    int rc;
    if ((rc = buf_ensure(c, BUF_T2, Mz * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_META2, Mz * sizeof(int)))) return rc;
    if ((rc = buf_ensure(c, BUF_MEAN, Mz * sizeof(float)))) return rc;
    if ((rc = buf_ensure(c, BUF_VAR, Mz * sizeof(float)))) return rc;
    if (M > 0) {
        HIPCHK(c, hipMemcpyAsync(buf<double>(c, BUF_T2), ht2.data(), sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(buf<int>(c, BUF_META2), hm2.data(), sizeof(int) * M, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = upload_table(c, BUF_TILES, tiles))) return rc;
    return buf_ensure(c, BUF_WORK, work_need);   // (0 for a call without tiles)
}

// k_pjvp_solve on nt tiles of the view V (kernels_posterior_jvp.h): W = P K* and V = L^-1 K* into the tiles' work rows, the fp32 mean
// and var into BUF_MEAN / BUF_VAR.  nvec = 0 (and null pointers): no derivative output is touched.
void launch_pjvp_solve(medgp_ctx *c, const MedgpDev &V, const PostTile *tiles, int nt, size_t stride, int nvec, double *d_dmean, double *d_dvar) {
    Launcher l(c, KID_PJ_SOLVE);
    hipLaunchKernelGGL(k_pjvp_solve, dim3(nt), dim3(256), 0, c->stream, V, tiles, buf<int>(c, BUF_META2), buf<double>(c, BUF_T2), buf<double>(c, BUF_WORK),
                       stride, nvec, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), d_dmean, d_dvar);
}
// "solve, then the family's kernel": per launch chunk of T (build_pjvp_tiles), in stream order -- the chunks reuse the work rows --
// k_pjvp_solve with nvec = 0, then f(chunk, its size class, the class view, its tiles on the device) launches what reads V
template <class F>
void for_solved_chunks(medgp_ctx *c, const BatchPlan &P, const PointTables<PostTile> &T, F &&f) {
    for (const TileChunk &ch : T.chunks) {
        const SizeClass &k = P.cls[ch.cls];
        const MedgpDev V = class_view(c, P, k);
        const PostTile *tiles = buf<PostTile>(c, BUF_TILES) + ch.t0;
        launch_pjvp_solve(c, V, tiles, ch.nt, ch.stride, 0, nullptr, nullptr);
        f(ch, k, V, tiles);
    }
}

// Two per-point arrays of n values each (fp32 [mean | var] from BUF_MEAN / BUF_VAR, an fp64 pair from a buffer of the call) on their
// way home; a call without points, or one the caller wants nothing of (a null), queues nothing.  sorted: the device's point order is
// not the caller's (forecast, VJP) -- the values land there, and once the stream has been waited for unsort_pair carries value k to the
// caller's point src[k].
template <class T>
int download_pair(medgp_ctx *c, int64_t n, const T *d_a, const T *d_b, T *a, T *b, std::vector<T> *sorted = nullptr) {
    if (n <= 0 || !a) return MEDGP_OK;
    if (sorted) { sorted->resize(2 * (size_t)n); a = sorted->data(); b = a + n; }
    HIPCHK(c, hipMemcpyAsync(a, d_a, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(b, d_b, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
    return MEDGP_OK;
}
template <class T>
void unsort_pair(const std::vector<T> &sorted, const int64_t *src, T *a, T *b) {
    const size_t n = sorted.size() / 2;
    for (size_t k = 0; k < n; k++) { a[src[k]] = sorted[k]; b[src[k]] = sorted[n + k]; }
}

// ---- what the derivative entry points share on top of that (the gradient objectives, Fisher / Hessian products, posterior JVP / VJP,
// ---- the baseline, basis and warp calls; launch_slabsum, launch_epilogue, finish_objective_class, launch_tiles and launch_wgrad stand
// ---- next to Launcher; the test-point side of the calls that have one is the block above: check_points ... unsort_pair) ----------
// The tile kernels of these calls are instantiated for Q <= 16 only.  why: what the generic route would break in the call (null: nothing said).
static_assert(PJVP_MAX_Q == 16, "the column tables of the JVP / VJP tile kernels are sized for what check_q16 lets through");
int check_q16(medgp_ctx *c, const char *who, const char *why) {
    if (c->rules.Q <= 16) return MEDGP_OK;
    return fail(c, MEDGP_ERR_ARG, "%s supports Q <= 16 (Q = %d)%s%s", who, c->rules.Q, why ? ": " : "", why ? why : "");
}
const char *const kWhyKinv = "the generic gradient route keeps W in the buffer that holds K^-1 here";

// The nmats matrices of every entry of the call are alive at once: the plan has one memory wave and the call's own buffers fit beside
// it (fits: the call's rule, *_tables.h).  suffix: what else the rule counts, for the message.
int check_one_wave(medgp_ctx *c, bool fits, int nmats, const char *suffix) {
    if (c->plan.nwaves == 1 && fits) return MEDGP_OK;
    return fail(c, MEDGP_ERR_CAPACITY,
                "the call's per-entry matrices (%d of %zu MB)%s exceed the memory budget of %zu MB (MEDGP_MEM_BUDGET_GB): split the call",
                nmats, (c->plan.need_mat * sizeof(double)) >> 20, suffix, c->rules.mem_budget >> 20);
}

// These calls leave their results in lane 0's staging (d_nlml, d_grad, d_status_out): a download of that lane still in flight on the copy
// stream must have read it first.
int wait_lane0_staging(medgp_ctx *c) {
    if (c->lane_pending[0] && c->ev_lane[0]) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_lane[0], 0));
    return MEDGP_OK;
}

// factor_run of a derivative call: theta to the device and the one pipeline run with U = L^-T and alpha, always on the templated
// kernels.  The generic ones (MEDGP_V0) are not honoured: their gradient route keeps W in the block of Kmat where these calls put
// K^-1 (the forecast gradient: Qm), and the second pass of every call is instantiated for the templated route alone.
int factor_run_templated(medgp_ctx *c, int nbatch, const double *theta, int min_n = 1) {
    const bool v0 = c->rules.use_v0;
    c->rules.use_v0 = false;
    const int rc = factor_run(c, nbatch, theta, true, false, min_n);
    c->rules.use_v0 = v0;
    return rc;
}

// P = K^-1 = U U^T of the entries of class k into the dead Kmat block (kernels_loo_grad.h)
void launch_kinv(medgp_ctx *c, const BatchPlan &P, const SizeClass &k, const MedgpDev &V) {
    const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, k.count, k.nbmax);
    Launcher l(c, KID_LOO_KINV);
    hipLaunchKernelGGL(k_loo_kinv, dim3(wg.grid), dim3(WG_THREADS), 0, c->stream, V, k.count, wg.wg_tiles, wg.nbp);
}
// Kdot of direction j of nvec of class k (kernels_fisher.h): the direction's coefficients into cf, then the matrix into Kd
void launch_kdot(medgp_ctx *c, const MedgpDev &V, const SizeClass &k, const double *d_dir, int nvec, int j, double *cf, double *Kd) {
    {
        Launcher l(c, KID_FI_PREP);
        hipLaunchKernelGGL(k_fisher_prep, dim3(k.count, 1 + (V.Q * V.D * V.D + 255) / 256), dim3(256), 0, c->stream, V, c->d_theta, d_dir, nvec, j, cf);
    }
    Launcher l(c, KID_FI_KDOT);   // (Q <= 16 was checked)
    with_q16(V.Q, [&](auto q, auto q0) {
        hipLaunchKernelGGL((k_fisher_kdot<decltype(q)::value, decltype(q0)::value>), dim3(fisher_kdot_grid(k.nbmax), k.count), dim3(256), 0, c->stream, V, cf, Kd);
    });
}
// T = P Kdot of class k (kernels_fisher.h)
void launch_fisher_t(medgp_ctx *c, const MedgpDev &V, const SizeClass &k, const double *Kd, double *Tm) {
    Launcher l(c, KID_FI_T);
    hipLaunchKernelGGL(k_fisher_t, dim3(fisher_t_grid(k.nbmax), k.count), dim3(WG_THREADS), 0, c->stream, V, Kd, Tm, k.nbmax);
}

// The end of a blocking call whose epilogue wrote lane 0's staging: objective, gradient (flag_grad) and status of the caller's rows to
// the host (null: not wanted), with one more block of the call's own (extra_bytes of extra_src -> extra_dst; 0: none) behind them;
// the stream is waited for and the blocks outgrown arenas left behind are freed.
int download_objective(medgp_ctx *c, int nbatch, int flag_grad, double *obj, double *grad, int32_t *status,
                       void *extra_dst = nullptr, const void *extra_src = nullptr, size_t extra_bytes = 0) {
    if (obj) HIPCHK(c, hipMemcpyAsync(obj, c->d_nlml, sizeof(double) * nbatch, hipMemcpyDeviceToHost, c->stream));
    if (flag_grad && grad) HIPCHK(c, hipMemcpyAsync(grad, c->d_grad, sizeof(double) * nbatch * c->H, hipMemcpyDeviceToHost, c->stream));
    if (status) HIPCHK(c, hipMemcpyAsync(status, c->d_status_out, sizeof(int32_t) * nbatch, hipMemcpyDeviceToHost, c->stream));
    if (extra_bytes) HIPCHK(c, hipMemcpyAsync(extra_dst, extra_src, extra_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_retired(c);
    return MEDGP_OK;
}

// The per-direction outputs of a call, [nvec][nbatch][H] on the device (count doubles: the call's *_tables.h rule): download_directions
// queues their way to `out`; once the stream has been waited for, transpose_directions lays them out as the caller takes them,
// [nbatch][nvec][H].
int download_directions(medgp_ctx *c, const double *d_out, size_t count, std::vector<double> &out) {
    out.resize(count);
    HIPCHK(c, hipMemcpyAsync(out.data(), d_out, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return MEDGP_OK;
}
void transpose_directions(const std::vector<double> &out, int nbatch, int nvec, size_t H, double *dst) {
    for (int b = 0; b < nbatch; b++)
        for (int j = 0; j < nvec; j++)
            std::memcpy(dst + ((size_t)b * nvec + j) * H, out.data() + ((size_t)j * nbatch + b) * H, H * sizeof(double));
}

}  // namespace

extern "C" {

int medgp_abi_version(void) { return 23; }

int medgp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *medgp_last_error(const medgp_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int medgp_create(medgp_ctx **out, int device, int kernel_index, int Q, int D, int R) {
    if (!out) return fail(nullptr, MEDGP_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (kernel_index == MEDGP_KERNEL_SE) { Q = 1; D = 1; R = 0; }
    if (kernel_index == MEDGP_KERNEL_SM) { D = 1; R = 0; }
    int nc = num_cov(kernel_index, Q, D, R);
    if (nc < 0) return fail(nullptr, MEDGP_ERR_ARG, "unsupported kernel_index %d (supported: 0 SE, 7 LMC-SM, 8 SM)", kernel_index);
    if (Q < 1 || D < 1 || R < 0) return fail(nullptr, MEDGP_ERR_ARG, "bad Q/D/R = %d/%d/%d", Q, D, R);
    if (D > MEDGP_MAX_D) return fail(nullptr, MEDGP_ERR_ARG, "D = %d exceeds the supported %d outputs", D, MEDGP_MAX_D);
    int ndev = medgp_device_count();
    if (ndev <= 0) return fail(nullptr, MEDGP_ERR_NODEVICE, "no HIP device visible; libmedgp_hip has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, MEDGP_ERR_ARG, "device %d outside [0, %d)", device, ndev);
    medgp_ctx *c = new medgp_ctx();
    c->device = device;
    c->kidx = kernel_index; c->rules.Q = Q; c->rules.D = D; c->R = R;
    c->nlik = (kernel_index == MEDGP_KERNEL_LMC_SM) ? D : 1;
    c->H = c->nlik + nc;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(nullptr, MEDGP_ERR_HIP, "cannot initialise device %d", device);
    }
    c->stream = c->own_stream;
    { const char *e = getenv("MEDGP_CHOLINV_NW"); c->rules.cholinv_nw = e ? atoi(e) : 0; }
    { const char *e = getenv("MEDGP_LA_PARK"); if (e) c->la_park = atoi(e); }
    { const char *e = getenv("MEDGP_LA_PARK_MAXBATCH"); if (e) c->la_park_maxbatch = atoi(e); }
    { const char *e = getenv("MEDGP_MULTI_CU"); c->rules.force_mc = e ? atoi(e) : 0; }
    { const char *e = getenv("MEDGP_CLASS_STREAMS"); if (e) c->class_streams = std::max(0, std::min(kAuxStreams, atoi(e))); }
    { const char *e = getenv("MEDGP_NO_CLASSES"); c->rules.no_classes = e ? atoi(e) : 0; }
    { const char *e = getenv("MEDGP_WGRAD_DEEP"); c->wgrad_deep = e ? std::max(1, atoi(e)) : -1; }
    { const char *e = getenv("MEDGP_DEBUG_FAIL_ATTEMPTS"); c->dbg_fail = e ? atoi(e) : 0; }
    { const char *e = getenv("MEDGP_V0"); c->rules.use_v0 = e && e[0] == '1'; }
    { const char *e = getenv("MEDGP_MEM_BUDGET_GB"); if (e && atof(e) > 0) c->rules.mem_budget = (size_t)(atof(e) * 1073741824.0); }
    { const char *e = getenv("MEDGP_SCREEN_LANES"); if (e && atoi(e) >= 1) c->rules.screen_lanes = std::min(2, atoi(e)); }
    { const char *e = getenv("MEDGP_SCREEN_WORK"); if (e && atoll(e) > 0) c->rules.screen_work = atoll(e); }
    { const char *e = getenv("MEDGP_SCREEN_BUDGET_GB"); if (e && atof(e) > 0) c->rules.screen_budget = (size_t)(atof(e) * 1073741824.0); }
    { const char *e = getenv("MEDGP_POSTERIOR_BUDGET_GB"); if (e && atof(e) > 0) c->posterior_budget = (size_t)(atof(e) * 1073741824.0); }
    for (int i = 0; i < kAuxStreams; i++) {
        (void)hipStreamCreateWithFlags(&c->aux[i], hipStreamNonBlocking);
        (void)hipEventCreateWithFlags(&c->ev_join[i], hipEventDisableTiming);
    }
    (void)hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    (void)hipStreamCreateWithFlags(&c->s_screen1, hipStreamNonBlocking);
    for (hipEvent_t *e : {&c->ev_fork1, &c->ev_screen0}) (void)hipEventCreateWithFlags(e, hipEventDisableTiming);
    { hipDeviceProp_t pr; if (hipGetDeviceProperties(&pr, device) == hipSuccess) c->rules.num_cu = pr.multiProcessorCount; }
    *out = c;
    return MEDGP_OK;
}

void medgp_destroy(medgp_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &e : c->events) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    free_all(c);
    for (int i = 0; i < kAuxStreams; i++) {
        if (c->aux[i]) { (void)hipStreamSynchronize(c->aux[i]); (void)hipStreamDestroy(c->aux[i]); }
        if (c->ev_join[i]) (void)hipEventDestroy(c->ev_join[i]);
    }
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->s_screen1) { (void)hipStreamSynchronize(c->s_screen1); (void)hipStreamDestroy(c->s_screen1); }
    for (hipEvent_t e : {c->ev_fork1, c->ev_screen0}) if (e) (void)hipEventDestroy(e);
    if (c->h_screen_tab) (void)hipHostFree(c->h_screen_tab);
    for (hipStream_t st : {c->s_up, c->s_down}) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (int i = 0; i < 2; i++) { if (c->ev_up[i]) (void)hipEventDestroy(c->ev_up[i]); if (c->ev_k[i]) (void)hipEventDestroy(c->ev_k[i]); }
    if (c->ev_stage) (void)hipEventDestroy(c->ev_stage);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->ev_basis) (void)hipEventDestroy(c->ev_basis);
    if (c->h_basis_stage) (void)hipHostFree(c->h_basis_stage);
    if (c->h_bounce) (void)hipHostFree(c->h_bounce);
    if (c->h_small) (void)hipHostFree(c->h_small);
    if (c->d_small) (void)hipFree(c->d_small);
    for (int i = 0; i < 2; i++) {
        if (c->pin_buf[i]) (void)hipHostFree(c->pin_buf[i]);
        if (c->pin_ev[i]) (void)hipEventDestroy(c->pin_ev[i]);
        if (c->ev_lane[i]) (void)hipEventDestroy(c->ev_lane[i]);
    }
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int medgp_num_hyp(const medgp_ctx *c) { return c ? c->H : MEDGP_ERR_ARG; }

int medgp_set_pi(medgp_ctx *c, double pi) {
    if (!c || !(pi > 0)) return MEDGP_ERR_ARG;
    c->pi = pi;
    c->dev.pi = pi;
    return MEDGP_OK;
}

int medgp_set_stream(medgp_ctx *c, void *s) {
    if (!c) return MEDGP_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return MEDGP_OK;
}

int medgp_synchronize(medgp_ctx *c) {
    if (!c) return MEDGP_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->s_down) HIPCHK(c, hipStreamSynchronize(c->s_down));   // (result downloads of the asynchronous lanes)
    free_retired(c);   // (every kernel of the context is queued on, or joined into, its stream: idle now)
    return MEDGP_OK;
}

int medgp_reserve(medgp_ctx *c, int max_slots, int max_n, int max_batch) {
    if (!c) return MEDGP_ERR_ARG;
    if (max_slots < 1 || max_n < 1 || max_batch < 1) return fail(c, MEDGP_ERR_ARG, "medgp_reserve: non-positive capacity");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_all(c);
    c->max_slots = max_slots; c->max_n = max_n; c->rules.max_batch = max_batch;
    // leading dimension = padded n.  (Padding it off the power of two was measured: no effect -- the HBM channel hash
    // already spreads the 4096-byte row stride.)
    const int ldn = medgp_roundup(max_n, 64);
    c->ldn = ldn;
    const size_t S = max_slots, B = max_batch, Q = c->rules.Q, D = c->rules.D, H = c->H;
    int rc;
    // patient rows: [0, S) grouped by output (what the gradient kernels need); [S, 2S) the same patient in the CALLER's
    // observation order, filled only when that order is not already grouped (used for caller-order factors)
    if ((rc = dalloc(c, &c->d_pn, 2 * S))) return rc;
    if ((rc = dalloc(c, &c->d_pt, 2 * S * ldn))) return rc;
    if ((rc = dalloc(c, &c->d_py, 2 * S * ldn))) return rc;
    if ((rc = dalloc(c, &c->d_pmeta, 2 * S * ldn))) return rc;
    if ((rc = dalloc(c, &c->d_pseg, 2 * S * (D + 1)))) return rc;
    if ((rc = dalloc(c, &c->d_proff, 2 * S * (D + 1)))) return rc;
    if ((rc = dalloc(c, &c->d_pcoff, 2 * S * (D + 1)))) return rc;
    if ((rc = dalloc(c, &c->d_one_slot, 1))) return rc;
    if ((rc = dalloc(c, &c->d_prior, S * H))) return rc;
    if ((rc = dalloc(c, &c->d_prior_on, S))) return rc;
    if ((rc = dalloc(c, &c->d_bslot, B))) return rc;
    if ((rc = dalloc(c, &c->d_bpos, B))) return rc;
    if ((rc = dalloc(c, &c->d_tpos, B))) return rc;
    c->d_screen_theta = nullptr; c->screen_theta_cap = 0; c->tpos_on = false;   // (freed by free_all above)
    if ((rc = dalloc(c, &c->d_status, B))) return rc;
    if ((rc = dalloc(c, &c->d_jit, B))) return rc;
    if ((rc = dalloc(c, &c->d_bn, B))) return rc;
    if ((rc = dalloc(c, &c->d_theta, B * H))) return rc;
    if ((rc = dalloc(c, &c->d_nlml, B))) return rc;
    if ((rc = dalloc(c, &c->d_grad, B * H))) return rc;
    if ((rc = dalloc(c, &c->d_status_out, B))) return rc;
    if ((rc = dalloc(c, &c->d_theta1, B * H))) return rc;
    if ((rc = dalloc(c, &c->d_nlml1, B))) return rc;
    if ((rc = dalloc(c, &c->d_grad1, B * H))) return rc;
    if ((rc = dalloc(c, &c->d_status1, B))) return rc;
    c->lane_pending[0] = c->lane_pending[1] = false;
    c->d_prior_stage = nullptr; c->d_prior_slots = nullptr; c->prior_stage_rows = 0;   // freed by free_all above
    MedgpDev &L = c->dev;
    L.kidx = c->kidx; L.Q = c->rules.Q; L.D = c->rules.D; L.R = c->R; L.H = c->H; L.nlik = c->nlik;
    L.ldn = ldn; L.pld = ldn; L.max_slots = max_slots; L.max_batch = max_batch;
    L.bpos = nullptr;
    L.tpos = nullptr;
    L.hyp_stride = (int)(D + Q * D * D + 2 * Q);
    L.pi = c->pi;
    L.dbg_fail = c->dbg_fail;
    double *hyp, *scal, *Sb, *SMb, *SVb;
    const SlabGeom sg = slab_geom(ldn, c->rules.Q, c->rules.D);
    L.slab_R = sg.R; L.slab_C = sg.C; L.slab_stride = sg.stride;
    c->full_mat = B * ldn * ldn; c->full_vec = B * ldn; c->full_tab = B * Q * ldn; c->full_slab = B * L.slab_stride;
    L.Kmat = L.Linv = L.z = L.alpha = L.wdiag = L.cs = L.sn = L.slab = nullptr;
    {   // a wave of a call never uses more than the budget, and the budget never more than 70 % of what the device has free now
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0) {
            c->rules.mem_budget = std::min(c->rules.mem_budget, fr / 10 * 7);
            c->rules.screen_budget = std::min(c->rules.screen_budget, c->rules.mem_budget);
        }
    }
    // every configuration whose capacities stay below 8 GB of matrices (all of BASELINE.json's) is allocated in full here; beyond that
    // (a ragged cohort: max_batch x max_n^2 would not fit) the arenas start as token blocks and are sized by medgp_reserve_plan, or grow with the calls
    if (2 * c->full_mat * sizeof(double) <= kArenaEager) rc = ensure_arena(c, c->full_mat, c->full_mat, c->full_vec, c->full_tab, c->full_slab, true);
    else rc = ensure_arena(c, 0, 0, 0, 0, 0, true);   // (a token block each: the views never hold null pointers)
    if (rc) return rc;
    double *xk;
    if ((rc = dalloc(c, &xk, B * 64 * 64))) return rc;
    L.xk = xk; L.jit = c->d_jit; L.bn = c->d_bn;
    if ((rc = dalloc(c, &hyp, B * L.hyp_stride))) return rc;
    if ((rc = dalloc(c, &scal, B * 4))) return rc;
    if ((rc = dalloc(c, &L.epi_lp, B * MEDGP_EPI_PARTS))) return rc;
    if ((rc = dalloc(c, &L.epi_ticket, B))) return rc;
    HIPCHK(c, hipMemsetAsync(L.epi_ticket, 0, B * sizeof(int), c->stream));
    if ((rc = dalloc(c, &Sb, B * Q * D * D))) return rc;
    if ((rc = dalloc(c, &SMb, B * Q * D * D))) return rc;
    if ((rc = dalloc(c, &SVb, B * Q * D * D))) return rc;
    L.pn = c->d_pn; L.pt = c->d_pt; L.py = c->d_py; L.pmeta = c->d_pmeta; L.pseg = c->d_pseg;
    L.proff = c->d_proff; L.pcoff = c->d_pcoff;
    L.prior = c->d_prior; L.prior_on = c->d_prior_on; L.bslot = c->d_bslot;
    L.hyp = hyp; L.scal = scal;
    L.status = c->d_status; L.S = Sb; L.SM = SMb; L.SV = SVb;
    HIPCHK(c, hipMemsetAsync(c->d_prior_on, 0, S, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_pn, 0, 2 * S * sizeof(int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->h_n.assign(max_slots, -1);
    c->h_perm.assign(max_slots, {});
    c->h_perm_identity.assign(max_slots, 1);
    c->basis = BasisStore{};
    c->basis.slot.assign(max_slots, BasisSlot{});
    c->d_basis = nullptr;   // freed by free_all above
    c->basis_pending = false;
    c->d_slot_scale = nullptr;   // freed by free_all above
    c->h_has_scale.assign(max_slots, 0);
    L.nscale = nullptr;
    c->h_bslot.assign(max_batch, -1);
    c->last_nbatch = 0;
    c->plan = BatchPlan{};
    c->last_has_inverse = false;
    c->d_stage = nullptr;   // freed by free_all above
    if (c->h_stage) { (void)hipHostFree(c->h_stage); c->h_stage = nullptr; }
    c->stage_cap = 0;
    c->stage_pending = false;
    return MEDGP_OK;
}

int medgp_reserve_plan(medgp_ctx *c, int count, const int32_t *n, int ninit) {
    if (!c) return MEDGP_ERR_ARG;
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (count < 1 || !n || ninit < 0) return fail(c, MEDGP_ERR_ARG, "medgp_reserve_plan: bad argument");
    for (int i = 0; i < count; i++)
        if (n[i] < 0 || n[i] > c->max_n) return fail(c, MEDGP_ERR_CAPACITY, "medgp_reserve_plan: n[%d] = %d outside [0, %d]", i, n[i], c->max_n);
    HIPCHK(c, hipSetDevice(c->device));
    // largest first, as medgp_screen walks them and as the lock-step trainer admits them
    std::vector<int> ns(n, n + count);
    std::stable_sort(ns.begin(), ns.end(), [](int a, int b) { return a > b; });
    BatchPlan P;
    std::vector<LaNeed> las;
    std::vector<int> la_of;
    // (a) one nlml + gradient call over the announced patients (the largest max_batch of them)
    layout_plan(c->rules, ns.data(), std::min(count, c->rules.max_batch), true, P);
    PlanNeeds nd = plan_needs(c->rules, P, las, la_of);
    const size_t nu = nd.mat;   // (Linv: the screening chunks below are nlml-only plans and never touch it)
    // (b) the chunks medgp_screen forms of them (two lanes: twice the largest chunk)
    if (ninit > 0) {
        ScreenCut SC;
        screen_cut(c->rules, ns, ninit, SC);
        nd.raise(PlanNeeds{SC.cap_mat, SC.cap_vec, SC.cap_tab, 0, SC.cap_part, SC.cap_small}, SC.two ? 2 : 1);
    }
    int rc;
    if ((rc = ensure_arena(c, nd.mat, nu, nd.vec, nd.tab, nd.slab, true))) return rc;
    if (nd.la_part && (rc = arena_ensure(c, AR_LA_PART, nd.la_part * sizeof(double), 0, true, nullptr))) return rc;
    if (nd.la_small && (rc = arena_ensure(c, AR_LA_SMALL, nd.la_small * sizeof(double), 0, true, nullptr))) return rc;
    // a set-up call: wait for the context's streams once and give the replaced blocks back now, so that the loop that follows starts with
    // nothing left to release
    if (!c->retired.empty()) { if ((rc = sync_ctx_streams(c))) return rc; free_retired(c); }
    return MEDGP_OK;
}

int medgp_alloc_stats(const medgp_ctx *c, double *seconds, int64_t *calls, int64_t *arena_bytes) {
    if (!c) return MEDGP_ERR_ARG;
    if (seconds) *seconds = c->alloc_s;
    if (calls) *calls = c->alloc_calls;
    if (arena_bytes) { int64_t b = 0; for (int i = 0; i < AR_COUNT; i++) b += (int64_t)c->arena[i].bytes; *arena_bytes = b; }
    return MEDGP_OK;
}

// ---- patient upload: any number of patients are packed into one pinned staging buffer, copied with ONE H2D transfer and
// scattered into their padded slot rows by k_scatter_patients; nothing waits for the device (the staging buffer is
// guarded by an event that is only waited for when the next upload starts).
namespace {
struct UpEntry { int slot, n; const int32_t *meta; const float *t, *y; };

inline size_t up_payload_bytes(int n, int D) { return ((size_t)n * 20 + (size_t)(D + 1) * 12 + 7) & ~(size_t)7; }

int upload_patients(medgp_ctx *c, const std::vector<UpEntry> &ents) {
    const int D = c->rules.D, S = c->max_slots, ldn = c->ldn;
    const bool use_meta = (c->kidx == MEDGP_KERNEL_LMC_SM);
    // validate everything before touching any state
    std::vector<uint8_t> seen(ents.size() > 1 ? (size_t)S : 0, 0);
    for (const UpEntry &e : ents) {
        if (e.slot < 0 || e.slot >= S) return fail(c, MEDGP_ERR_CAPACITY, "slot %d outside [0, %d)", e.slot, S);
        if (!seen.empty()) {   // two scatter workgroups would write the same rows, and the host mirrors would keep whichever came last
            if (seen[e.slot]) return fail(c, MEDGP_ERR_ARG, "slot %d appears twice in one packed upload", e.slot);
            seen[e.slot] = 1;
        }
        if (e.n < 0 || e.n > c->max_n) return fail(c, MEDGP_ERR_CAPACITY, "n = %d outside [0, %d]", e.n, c->max_n);
        if (e.n > 0 && (!e.t || !e.y)) return fail(c, MEDGP_ERR_ARG, "t / y is NULL");
        if (use_meta && e.n > 0 && !e.meta) return fail(c, MEDGP_ERR_ARG, "meta is NULL for the multi-output kernel");
        if (use_meta)
            for (int i = 0; i < e.n; i++)
                if (e.meta[i] < 0 || e.meta[i] >= D) return fail(c, MEDGP_ERR_ARG, "meta[%d] = %d outside [0, %d)", i, e.meta[i], D);
    }
    // worst case: every patient also needs its caller-order copy
    size_t bytes = 0;
    for (const UpEntry &e : ents) bytes += 2 * (sizeof(MedgpUpHdr) + up_payload_bytes(e.n, D));
    HIPCHK(c, hipSetDevice(c->device));
    if (c->stage_pending) { HIPCHK(c, hipEventSynchronize(c->ev_stage)); c->stage_pending = false; }
    if (bytes > c->stage_cap) {
        const size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 16);
        if (c->h_stage) (void)hipHostFree(c->h_stage);
        c->h_stage = nullptr;
        HIPCHK(c, hipHostMalloc((void **)&c->h_stage, cap, hipHostMallocDefault));
        HIPCHK(c, hipStreamSynchronize(c->stream));   // the old device buffer may still be read by a queued scatter
        if (c->d_stage) {
            (void)hipFree(c->d_stage);
            c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void *)c->d_stage), c->allocs.end());
            c->d_stage = nullptr;
        }
        int rc = dalloc(c, &c->d_stage, cap);
        if (rc) return rc;
        c->stage_cap = cap;
    }
    if (!c->ev_stage) HIPCHK(c, hipEventCreateWithFlags(&c->ev_stage, hipEventDisableTiming));
    // count the device entries (grouped copy of every patient + caller-order copy of the ungrouped ones)
    std::vector<std::vector<int>> perms(ents.size());
    std::vector<uint8_t> ident(ents.size(), 1);
    int nent = 0;
    for (size_t k = 0; k < ents.size(); k++) {
        const UpEntry &e = ents[k];
        std::vector<int> &perm = perms[k];
        perm.resize(e.n);
        if (use_meta) {   // stable grouping by output (counting sort)
            std::vector<int> pos(D + 1, 0);
            for (int i = 0; i < e.n; i++) pos[e.meta[i] + 1]++;
            for (int d = 0; d < D; d++) pos[d + 1] += pos[d];
            for (int i = 0; i < e.n; i++) perm[pos[e.meta[i]]++] = i;
        } else {
            for (int i = 0; i < e.n; i++) perm[i] = i;
        }
        for (int i = 0; i < e.n; i++) if (perm[i] != i) { ident[k] = 0; break; }
        nent += ident[k] ? 1 : 2;
    }
    MedgpUpHdr *hdr = (MedgpUpHdr *)c->h_stage;
    size_t off = (size_t)nent * sizeof(MedgpUpHdr);
    int ie = 0;
    auto pack = [&](const UpEntry &e, int dev_slot, const int *perm) {
        hdr[ie].slot = dev_slot; hdr[ie].n = e.n; hdr[ie].off = (long long)off; ie++;
        double *pt = (double *)(c->h_stage + off), *py = pt + e.n;
        int *pm = (int *)(py + e.n), *seg = pm + e.n, *roff = seg + (D + 1), *coff = roff + (D + 1);
        for (int i = 0; i < e.n; i++) {
            const int src = perm ? perm[i] : i;
            pt[i] = (double)e.t[src];
            py[i] = (double)e.y[src];   // zero mean: ref mean/c_meanfunc_zero.cpp:32-50
            pm[i] = use_meta ? e.meta[src] : 0;
        }
        for (int d = 0; d <= D; d++) seg[d] = roff[d] = coff[d] = 0;
        if (perm || !use_meta) {   // grouped copy: output segments + slab slots of k_wgrad (16-row / 64-column pieces per output)
            if (use_meta) { for (int i = 0; i < e.n; i++) seg[pm[i] + 1]++; for (int d = 0; d < D; d++) seg[d + 1] += seg[d]; }
            else seg[1] = e.n;
            for (int d = 0; d < D; d++) {
                const int a = seg[d], z = seg[d + 1];
                roff[d + 1] = roff[d] + (z > a ? (z - 1) / 16 - a / 16 + 1 : 0);
                coff[d + 1] = coff[d] + (z > a ? (z - 1) / 64 - a / 64 + 1 : 0);
            }
        }
        off += up_payload_bytes(e.n, D);
    };
    for (size_t k = 0; k < ents.size(); k++) {
        pack(ents[k], ents[k].slot, perms[k].data());
        if (!ident[k]) pack(ents[k], ents[k].slot + S, nullptr);   // caller order (factor export / predict in that order)
    }
    HIPCHK(c, hipMemcpyAsync(c->d_stage, c->h_stage, off, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_stage, c->stream));
    c->stage_pending = true;
    hipLaunchKernelGGL(k_scatter_patients, dim3(nent), dim3(256), 0, c->stream, (const char *)c->d_stage, D, ldn, c->d_pn, c->d_pt,
                       c->d_py, c->d_pmeta, c->d_pseg, c->d_proff, c->d_pcoff);
    HIPCHK(c, hipGetLastError());
    for (size_t k = 0; k < ents.size(); k++) {
        const int s = ents[k].slot;
        c->h_n[s] = ents[k].n;
        c->h_perm[s] = std::move(perms[k]);
        c->h_perm_identity[s] = ident[k];
        c->basis.drop(s);   // its rows no longer belong to the data
        c->h_has_scale[s] = 0;   // ... and neither do its noise scales
    }
    c->last_nbatch = 0;   // cached batch selection / factors no longer describe the resident patients
    c->last_has_inverse = false;
    return MEDGP_OK;
}
}  // namespace

int medgp_set_patient(medgp_ctx *c, int slot, int n, const int32_t *meta, const float *t, const float *y) {
    if (!c) return MEDGP_ERR_ARG;
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    return upload_patients(c, {UpEntry{slot, n, meta, t, y}});
}

int medgp_set_patients(medgp_ctx *c, int nslots, const int32_t *slots, const int64_t *offsets, const int32_t *meta,
                       const float *t, const float *y) {
    if (!c) return MEDGP_ERR_ARG;
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (nslots < 1 || !slots || !offsets) return fail(c, MEDGP_ERR_ARG, "medgp_set_patients: bad argument");
    std::vector<UpEntry> ents(nslots);
    for (int k = 0; k < nslots; k++) {
        const int64_t a = offsets[k], z = offsets[k + 1];
        if (a < 0 || z < a || z - a > c->max_n) return fail(c, MEDGP_ERR_CAPACITY, "offsets[%d..%d] = %lld..%lld: bad length", k, k + 1, (long long)a, (long long)z);
        ents[k] = UpEntry{slots[k], (int)(z - a), meta ? meta + a : nullptr, t ? t + a : nullptr, y ? y + a : nullptr};
    }
    return upload_patients(c, ents);
}

namespace {
// rows: nrows descriptors of H hypers each (flag == NULL: "no prior"); slots == NULL: ONE row for every slot of the context.
// One pinned staging copy, one H2D transfer, one scatter kernel; nothing waits for the device.
int upload_priors(medgp_ctx *c, int nrows, const int32_t *slots, const uint8_t *flag, const int32_t *type, const uint8_t *is_exp,
                  const float *p0, const float *p1) {
    const int H = c->H;
    if (flag && (!type || !is_exp || !p0 || !p1)) return fail(c, MEDGP_ERR_ARG, "prior arrays must all be given");
    std::vector<uint8_t> seen((slots && nrows > 1) ? (size_t)c->max_slots : 0, 0);
    for (int k = 0; slots && k < nrows; k++) {
        if (slots[k] < 0 || slots[k] >= c->max_slots) return fail(c, MEDGP_ERR_CAPACITY, "slot %d outside [0, %d)", slots[k], c->max_slots);
        if (!seen.empty()) {   // two scatter workgroups would write the same prior rows: which one wins is undefined
            if (seen[slots[k]]) return fail(c, MEDGP_ERR_ARG, "slot %d appears twice in one medgp_set_priors", slots[k]);
            seen[slots[k]] = 1;
        }
    }
    if (flag)
        for (size_t h = 0; h < (size_t)nrows * H; h++)
            if (type[h] < -1 || type[h] > 2) return fail(c, MEDGP_ERR_ARG, "prior type[%zu] = %d unsupported (KDE prior type 3 is never constructed by the reference's mains)", h, type[h]);
    HIPCHK(c, hipSetDevice(c->device));
    if ((size_t)nrows > c->prior_stage_rows) {
        { int rcs = sync_ctx_streams(c); if (rcs) return rcs; }   // (the context's streams, not the device: other contexts keep running)
        for (void *q : {(void *)c->d_prior_stage, (void *)c->d_prior_slots})
            if (q) { (void)hipFree(q); c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), q), c->allocs.end()); }
        c->d_prior_stage = nullptr; c->d_prior_slots = nullptr; c->prior_stage_rows = 0;
        const size_t rows = std::max<size_t>(nrows, 16);
        int rc;
        if ((rc = dalloc(c, &c->d_prior_stage, rows * H))) return rc;
        if ((rc = dalloc(c, &c->d_prior_slots, rows))) return rc;
        c->prior_stage_rows = rows;
    }
    const size_t row_bytes = sizeof(MedgpPrior) * (size_t)H, slot_bytes = ((sizeof(int) * (size_t)nrows) + 15) & ~(size_t)15;
    void *pin = nullptr;
    int rc = pin_stage(c, slot_bytes + row_bytes * nrows, &pin);
    if (rc) return rc;
    int *hs = (int *)pin;
    MedgpPrior *hp = (MedgpPrior *)((char *)pin + slot_bytes);
    for (int k = 0; k < nrows; k++) {
        hs[k] = slots ? slots[k] : -1;
        for (int h = 0; h < H; h++) {
            MedgpPrior p{};
            const size_t e = (size_t)k * H + h;
            if (flag) {
                p.p0 = p0[e]; p.p1 = p1[e]; p.type = (int8_t)type[e]; p.flag = flag[e] ? 1 : 0; p.is_exp = is_exp[e] ? 1 : 0;
                if (type[e] == 2) p.lg2b = logf(2.0f * p1[e]);   // the reference's float log (MedgpPrior::lg2b)
            }
            else p.type = -1;
            hp[e] = p;
        }
    }
    if (slots) HIPCHK(c, hipMemcpyAsync(c->d_prior_slots, hs, sizeof(int) * nrows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_prior_stage, hp, row_bytes * nrows, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_scatter_priors, dim3(slots ? nrows : c->max_slots), dim3(256), 0, c->stream, (const MedgpPrior *)c->d_prior_stage,
                       slots ? (const int *)c->d_prior_slots : (const int *)nullptr, H, c->d_prior, c->d_prior_on, (uint8_t)(flag ? 1 : 0));
    HIPCHK(c, hipGetLastError());
    return MEDGP_OK;
}
}  // namespace

int medgp_set_prior(medgp_ctx *c, int slot, const uint8_t *flag, const int32_t *type, const uint8_t *is_exp,
                    const float *p0, const float *p1) {
    if (!c) return MEDGP_ERR_ARG;
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (slot < -1 || slot >= c->max_slots) return fail(c, MEDGP_ERR_CAPACITY, "slot %d outside [-1, %d)", slot, c->max_slots);
    const int32_t s1 = slot;
    return upload_priors(c, 1, slot < 0 ? nullptr : &s1, flag, type, is_exp, p0, p1);
}

int medgp_set_priors(medgp_ctx *c, int nslots, const int32_t *slots, const uint8_t *flag, const int32_t *type,
                     const uint8_t *is_exp, const float *p0, const float *p1) {
    if (!c) return MEDGP_ERR_ARG;
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (nslots < 1 || !slots) return fail(c, MEDGP_ERR_ARG, "medgp_set_priors: bad argument");
    return upload_priors(c, nslots, slots, flag, type, is_exp, p0, p1);
}

int medgp_nlml_grad_device(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta_dev, int flag_grad,
                           double *nlml_dev, double *grad_dev, int32_t *status_dev) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta_dev || !nlml_dev) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (flag_grad & ~(MEDGP_FLAG_GRAD | MEDGP_FLAG_KEEP_FACTOR)) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    const int grad = flag_grad & MEDGP_FLAG_GRAD;
    const bool keep = (flag_grad & MEDGP_FLAG_KEEP_FACTOR) != 0;
    if (grad && !grad_dev) return fail(c, MEDGP_ERR_ARG, "grad is NULL with flag_grad set");
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    // factor wanted but no gradient: patients that were not uploaded grouped by output are evaluated in the CALLER's order,
    // so that L^-1 is the factor the reference would hand to GP_Regression::predict (ref: core/gp_regression.cpp:181-196)
    if ((rc = set_batch(c, nbatch, slots, keep && !grad, grad || keep))) return rc;
    return run_pipeline(c, theta_dev, grad, keep, 3, nlml_dev, grad_dev, status_dev, false, keep);
}

int medgp_nlml_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int flag_grad, double *nlml,
                    double *grad, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !nlml) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if ((flag_grad & MEDGP_FLAG_GRAD) && !grad) return fail(c, MEDGP_ERR_ARG, "grad is NULL with flag_grad set");
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (nbatch < 1 || nbatch > c->rules.max_batch) return fail(c, MEDGP_ERR_CAPACITY, "nbatch %d outside [1, %d]", nbatch, c->rules.max_batch);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t H = c->H;
    const bool want_grad = (flag_grad & MEDGP_FLAG_GRAD) != 0;
    // Small calls (a few patients, the D = 2 configurations): the pageable copies of the runtime cost more than the kernels they
    // bracket (256 x N=256, D=2: 0.41 ms of kernels, 0.49 ms per call).  Up to 1 MB the arguments travel through pinned memory:
    // theta through the upload ring, the results into a pinned landing area, one host memcpy each.
    const size_t th_bytes = sizeof(double) * nbatch * H, out_bytes = sizeof(double) * nbatch * (1 + (want_grad ? H : 0)) + sizeof(int32_t) * nbatch;
    const size_t kSmall = (size_t)1 << 20;
    if (th_bytes <= kSmall && out_bytes <= kSmall) {
        if (!c->h_small) HIPCHK(c, hipHostMalloc((void **)&c->h_small, kSmall + 64, hipHostMallocDefault));
        if (!c->d_small) HIPCHK(c, hipMalloc((void **)&c->d_small, kSmall + 64));
        void *pin = nullptr;
        int rcp = pin_stage(c, th_bytes, &pin);
        if (rcp) return rcp;
        std::memcpy(pin, theta, th_bytes);
        HIPCHK(c, hipMemcpyAsync(c->d_theta, pin, th_bytes, hipMemcpyHostToDevice, c->stream));
        // the kernels write nlml, gradients and status into ONE device block laid out like the landing area: one copy instead of three
        // (each copy is a packet of its own on the stream: ~ 4 us apiece behind a 0.4 ms call)
        double *dn = (double *)c->d_small, *dg = dn + nbatch;
        int32_t *ds = (int32_t *)(dg + (want_grad ? (size_t)nbatch * H : 0));
        int rc = medgp_nlml_grad_device(c, nbatch, slots, c->d_theta, flag_grad, dn, want_grad ? dg : nullptr, ds);
        if (rc) return rc;
        double *hn = (double *)c->h_small, *hg = hn + nbatch;
        int32_t *hs = (int32_t *)(hg + (want_grad ? (size_t)nbatch * H : 0));
        HIPCHK(c, hipMemcpyAsync(hn, dn, out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memcpy(nlml, hn, sizeof(double) * nbatch);
        if (want_grad) std::memcpy(grad, hg, sizeof(double) * nbatch * H);
        if (status) std::memcpy(status, hs, sizeof(int32_t) * nbatch);
        free_retired(c);   // (the stream is idle: blocks that outgrown arenas left behind can go)
        return MEDGP_OK;
    }
    int rc;
    if ((rc = wait_lane0_staging(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_theta, theta, th_bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = medgp_nlml_grad_device(c, nbatch, slots, c->d_theta, flag_grad, c->d_nlml, c->d_grad, c->d_status_out))) return rc;
    return download_objective(c, nbatch, want_grad, nlml, grad, status);
}

int medgp_screen(medgp_ctx *c, int nslots, const int32_t *slots, int ninit, const double *theta, double *nlml, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !nlml || nslots < 1 || ninit < 1) return fail(c, MEDGP_ERR_ARG, "medgp_screen: bad argument");
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t H = c->H, total = (size_t)nslots * ninit;
    for (int s = 0; s < nslots; s++)
        if (slots[s] < 0 || slots[s] >= c->max_slots || c->h_n[slots[s]] < 0) return fail(c, MEDGP_ERR_ARG, "slots[%d] = %d is not a resident patient", s, slots[s]);
    if ((size_t)ninit * H > c->screen_theta_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_screen_theta) { (void)hipFree(c->d_screen_theta); c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void *)c->d_screen_theta), c->allocs.end()); c->d_screen_theta = nullptr; }
        int rc = dalloc(c, &c->d_screen_theta, (size_t)ninit * H);
        if (rc) return rc;
        c->screen_theta_cap = (size_t)ninit * H;
    }
    { int rc = wait_lane0_staging(c); if (rc) return rc; }
    HIPCHK(c, hipMemcpyAsync(c->d_screen_theta, theta, sizeof(double) * ninit * H, hipMemcpyHostToDevice, c->stream));
    // pinned landing area of all results: [nlml: total doubles | status: total ints]
    const size_t land = sizeof(double) * total + sizeof(int32_t) * total;
    if (land > c->bounce_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->h_bounce) (void)hipHostFree(c->h_bounce);
        c->h_bounce = nullptr; c->bounce_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->h_bounce, land + land / 4, hipHostMallocDefault));
        c->bounce_cap = land + land / 4;
    }
    double *hn = (double *)c->h_bounce;
    int32_t *hs = (int32_t *)(c->h_bounce + sizeof(double) * total);
    // The patients are walked LARGEST FIRST whatever the caller's order (results go back to the caller's rows at the end): a chunk that
    // holds the last vectors of one patient and the first of the next then holds two patients of similar size -- one size class, one
    // launch set -- where the caller's order (the trainer's read-ahead delivers patients as its readers finish) would put a handful of
    // entries of a very different size into a class and a kernel chain of their own: measured on the 512-patient heavy-tailed cohort,
    // 1000 vectors each: 8.7-11.3 s in arrival order against 5.0 s sorted.
    std::vector<int> perm(nslots);
    for (int s = 0; s < nslots; s++) perm[s] = s;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return c->h_n[slots[a]] > c->h_n[slots[b]]; });
    std::vector<int> walk_n(nslots);
    for (int s = 0; s < nslots; s++) walk_n[s] = c->h_n[slots[perm[s]]];
    // ---- chunks of consecutive (patient, vector) entries (screen_chunk_end).  ONE chunk (everything fits one call): the context's own
    // plan on its own stream, exactly the call medgp_nlml_grad(flag_grad = 0) makes of the same entries.  SEVERAL chunks: they
    // alternate between two LANES -- two streams, each with its own rows of the batch-indexed buffers, its own half of the arenas and
    // its own auxiliary streams -- so that the assembly of one chunk (fp64 VALU bound) runs beside the factorisation of the other (MFMA
    // + latency bound) and the tail of one chunk's launch is filled by the other's.  Measured before it was built, with two contexts
    // screening the same patient at once: 2.24 against 2.48 ms per 1000 evaluations at N = 512 (scratch/screen_two_ctx.py).  A chunk of a
    // two-lane call holds at most max_batch / 2 entries (its rows of the buffers).
    ScreenCut SC;
    screen_cut(c->rules, walk_n, ninit, SC);
    const bool two = SC.two;
    const std::vector<ScreenChunk> &chunks = SC.chunks;
    const int lane_rows = SC.lane_rows;
    const size_t cap_mat = SC.cap_mat, cap_vec = SC.cap_vec, cap_tab = SC.cap_tab, cap_part = SC.cap_part, cap_small = SC.cap_small;
    BatchPlan lane_plan[2];
    if (two) {
        int rc0;
        if ((rc0 = ensure_arena(c, 2 * cap_mat, 0, 2 * cap_vec, 2 * cap_tab, 0))) return rc0;
        if (cap_part && (rc0 = arena_ensure(c, AR_LA_PART, 2 * cap_part * sizeof(double), 0, false, nullptr))) return rc0;
        if (cap_small && (rc0 = arena_ensure(c, AR_LA_SMALL, 2 * cap_small * sizeof(double), 0, false, nullptr))) return rc0;
        // the tables of ALL chunks in one pinned block: a lane's copies read their own region, which nobody rewrites during the call
        // (the two-buffer upload ring is guarded by events on c->stream only)
        const size_t tab_bytes = sizeof(int) * 3 * total;
        if (tab_bytes > c->screen_tab_cap) {
            { int rcs = sync_ctx_streams(c); if (rcs) return rcs; }
            if (c->h_screen_tab) (void)hipHostFree(c->h_screen_tab);
            c->h_screen_tab = nullptr; c->screen_tab_cap = 0;
            HIPCHK(c, hipHostMalloc((void **)&c->h_screen_tab, tab_bytes + tab_bytes / 4, hipHostMallocDefault));
            c->screen_tab_cap = tab_bytes + tab_bytes / 4;
        }
        // lane 1 starts behind everything queued on the context's stream so far (the theta block, earlier calls that use the arenas)
        HIPCHK(c, hipEventRecord(c->ev_screen0, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->s_screen1, c->ev_screen0, 0));
    }
    std::vector<int32_t> cs;
    std::vector<int> tp, en;
    int rc = MEDGP_OK;
    c->tpos_on = true;
    for (size_t ci = 0; ci < chunks.size() && rc == MEDGP_OK; ci++) {
        const size_t e0 = chunks[ci].e0, e1 = chunks[ci].e1;
        const int nb = (int)(e1 - e0);
        cs.clear(); tp.clear();
        for (size_t x = e0; x < e1; x++) { cs.push_back(slots[perm[x / ninit]]); tp.push_back((int)(x % ninit)); }
        hipError_t he = hipSuccess;
        if (!two) {
            if ((rc = set_batch(c, nb, cs.data(), false, false))) break;
            {   // theta rows in the plan's internal order
                void *pin = nullptr;
                if ((rc = pin_stage(c, sizeof(int) * nb, &pin))) break;
                int *hp = (int *)pin;
                for (int i = 0; i < nb; i++) hp[i] = tp[c->plan.order[i]];
                he = hipMemcpyAsync(c->d_tpos, hp, sizeof(int) * nb, hipMemcpyHostToDevice, c->stream);
                if (he != hipSuccess) { rc = fail(c, MEDGP_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(he)); break; }
            }
            if ((rc = run_pipeline(c, c->d_screen_theta, 0, false, 3, c->d_nlml, nullptr, c->d_status_out))) break;
            he = hipMemcpyAsync(hn + e0, c->d_nlml, sizeof(double) * nb, hipMemcpyDeviceToHost, c->stream);
            if (he == hipSuccess) he = hipMemcpyAsync(hs + e0, c->d_status_out, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, c->stream);
        } else {
            const int lane = (int)(ci & 1);
            hipStream_t st = lane ? c->s_screen1 : c->stream;
            BatchPlan &P = lane_plan[lane];
            en.resize(nb);
            for (int i = 0; i < nb; i++) en[i] = c->h_n[cs[i]];
            layout_plan(c->rules, en.data(), nb, false, P);
            P.row0 = lane * lane_rows;
            P.mat0 = lane * cap_mat; P.vec0 = lane * cap_vec; P.tab0 = lane * cap_tab; P.la_part0 = lane * cap_part; P.la_small0 = lane * cap_small;
            int *hb = (int *)c->h_screen_tab + 3 * e0, *hpz = hb + nb, *ht = hpz + nb;
            for (int i = 0; i < nb; i++) { hb[i] = cs[P.order[i]]; hpz[i] = P.order[i]; ht[i] = tp[P.order[i]]; }
            he = hipMemcpyAsync(c->d_bslot + P.row0, hb, sizeof(int) * nb, hipMemcpyHostToDevice, st);
            if (he == hipSuccess) he = hipMemcpyAsync(c->d_bpos + P.row0, hpz, sizeof(int) * nb, hipMemcpyHostToDevice, st);
            if (he == hipSuccess) he = hipMemcpyAsync(c->d_tpos + P.row0, ht, sizeof(int) * nb, hipMemcpyHostToDevice, st);
            if (he != hipSuccess) { rc = fail(c, MEDGP_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(he)); break; }
            if ((rc = run_pipeline(c, c->d_screen_theta, 0, false, 3, c->d_nlml + P.row0, nullptr, c->d_status_out + P.row0, false, false,
                                   &P, st, lane * (kAuxStreams / 2), kAuxStreams / 2, lane ? c->ev_fork1 : c->ev_fork))) break;
            he = hipMemcpyAsync(hn + e0, c->d_nlml + P.row0, sizeof(double) * nb, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipMemcpyAsync(hs + e0, c->d_status_out + P.row0, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st);
        }
        if (he != hipSuccess) { rc = fail(c, MEDGP_ERR_HIP, "hipMemcpyAsync failed: %s", hipGetErrorString(he)); break; }
    }
    c->tpos_on = false;
    c->last_nbatch = 0;   // (the cached plan carries this call's theta rows: the next call lays its own out)
    if (two) {
        c->plan = lane_plan[0];   // (diagnostics: medgp_last_plan reports lane 0's last chunk)
        c->last_has_inverse = false;
        HIPCHK(c, hipStreamSynchronize(c->s_screen1));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_retired(c);
    if (rc) return rc;
    for (int sp = 0; sp < nslots; sp++) {   // walk order -> the caller's rows
        std::memcpy(nlml + (size_t)perm[sp] * ninit, hn + (size_t)sp * ninit, sizeof(double) * ninit);
        if (status) std::memcpy(status + (size_t)perm[sp] * ninit, hs + (size_t)sp * ninit, sizeof(int32_t) * ninit);
    }
    return MEDGP_OK;
}

void *medgp_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void medgp_host_free(void *p) { if (p) (void)hipHostFree(p); }

int medgp_nlml_grad_async(medgp_ctx *c, int lane, int nbatch, const int32_t *slots, const double *theta, int flag_grad,
                          double *nlml, double *grad, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (lane < 0 || lane > 1) return fail(c, MEDGP_ERR_ARG, "lane %d outside {0, 1}", lane);
    if (!slots || !theta || !nlml) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if ((flag_grad & MEDGP_FLAG_GRAD) && !grad) return fail(c, MEDGP_ERR_ARG, "grad is NULL with flag_grad set");
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (nbatch < 1 || nbatch > c->rules.max_batch) return fail(c, MEDGP_ERR_CAPACITY, "nbatch %d outside [1, %d]", nbatch, c->rules.max_batch);
    if (c->lane_pending[lane]) return fail(c, MEDGP_ERR_ARG, "lane %d still holds a call: medgp_wait it first", lane);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t H = c->H;
    double *dth = lane ? c->d_theta1 : c->d_theta, *dnl = lane ? c->d_nlml1 : c->d_nlml, *dgr = lane ? c->d_grad1 : c->d_grad;
    int *dst = lane ? c->d_status1 : c->d_status_out;
    if (!c->s_up) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_up, hipStreamNonBlocking));
        HIPCHK(c, hipStreamCreateWithFlags(&c->s_down, hipStreamNonBlocking));
    }
    for (hipEvent_t *e : {&c->ev_up[lane], &c->ev_k[lane], &c->ev_lane[lane]})
        if (!*e) HIPCHK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    // theta: on the upload stream (the lane's staging is free: the caller has waited for the lane's previous call)
    HIPCHK(c, hipMemcpyAsync(dth, theta, sizeof(double) * nbatch * H, hipMemcpyHostToDevice, c->s_up));
    HIPCHK(c, hipEventRecord(c->ev_up[lane], c->s_up));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_up[lane], 0));
    int rc = medgp_nlml_grad_device(c, nbatch, slots, dth, flag_grad, dnl, dgr, dst);
    if (rc) return rc;
    // results: on the download stream, behind this call's kernels
    HIPCHK(c, hipEventRecord(c->ev_k[lane], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->s_down, c->ev_k[lane], 0));
    HIPCHK(c, hipMemcpyAsync(nlml, dnl, sizeof(double) * nbatch, hipMemcpyDeviceToHost, c->s_down));
    if (flag_grad & MEDGP_FLAG_GRAD) HIPCHK(c, hipMemcpyAsync(grad, dgr, sizeof(double) * nbatch * H, hipMemcpyDeviceToHost, c->s_down));
    if (status) HIPCHK(c, hipMemcpyAsync(status, dst, sizeof(int32_t) * nbatch, hipMemcpyDeviceToHost, c->s_down));
    HIPCHK(c, hipEventRecord(c->ev_lane[lane], c->s_down));
    c->lane_pending[lane] = true;
    return MEDGP_OK;
}

int medgp_wait(medgp_ctx *c, int lane) {
    if (!c) return MEDGP_ERR_ARG;
    if (lane < 0 || lane > 1) return fail(c, MEDGP_ERR_ARG, "lane %d outside {0, 1}", lane);
    if (!c->lane_pending[lane]) return MEDGP_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ev_lane[lane]));
    c->lane_pending[lane] = false;
    return MEDGP_OK;
}

int medgp_get_factor(medgp_ctx *c, int b, float *alpha, float *linv, float *beta) {
    if (!c) return MEDGP_ERR_ARG;
    if (b < 0 || b >= c->last_nbatch) return fail(c, MEDGP_ERR_ARG, "batch entry %d outside the last call's [0, %d)", b, c->last_nbatch);
    if (!c->last_has_inverse)
        return fail(c, MEDGP_ERR_ARG, "no factor available: the last call formed neither gradients nor the factor "
                                      "(pass MEDGP_FLAG_GRAD or MEDGP_FLAG_KEEP_FACTOR to medgp_nlml_grad)");
    HIPCHK(c, hipSetDevice(c->device));
    const int S = c->max_slots;
    const MedgpDev E = entry_view(c, b);   // the entry's rows of the batch buffers (its size class's view, shifted)
    const int ld = E.ldn;
    int eff = c->h_bslot[b];
    const int slot = eff >= S ? eff - S : eff, n = c->h_n[slot];
    const std::vector<int> &perm = c->h_perm[slot];
    int st = 0;
    HIPCHK(c, hipMemcpyAsync(&st, E.status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (st < 0) return fail(c, MEDGP_ERR_ARG, "batch entry %d failed (status %d); no factor available", b, st);
    if (linv && eff < S && !c->h_perm_identity[slot]) {
        // The entry was factored in the grouped order (the gradient needs it), but L^-1 is order dependent: re-factor this
        // one entry from the caller-order copy of the patient (same hyper block; tables, Gram, factor and inverse redone).
        const int shadow = slot + S;
        HIPCHK(c, hipMemcpyAsync(c->d_one_slot, &shadow, sizeof(int), hipMemcpyHostToDevice, c->stream));
        MedgpDev V = E;
        V.bslot = c->d_one_slot;
        V.bpos = nullptr;
        const bool prof = c->profiling;
        c->profiling = false;   // not part of the evaluation being measured
        // its route: that of a call of this one entry (choose_routes on a one-entry plan)
        BatchPlan P1;
        std::vector<LaNeed> las;
        std::vector<int> la_of;
        std::vector<LaArgs> la;
        layout_plan(c->rules, &n, 1, true, P1);
        choose_routes(c->rules, P1, las, la_of);
        if (!las.empty()) {
            las[0].ld = ld;   // (the entry keeps the view of its class in the last call: the Y row block has that leading dimension)
            int rcl = ensure_la(c, las, true, la);
            if (rcl) return rcl;
        }
        const SizeClass &k1 = P1.cls[0];
        int rc = run_pipeline_one(c, c->stream, V, 1, k1.nbmax, nullptr, 0, true, 1, nullptr, nullptr, nullptr, false, &n, k1.route, la.empty() ? nullptr : &la[0]);
        c->profiling = prof;
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync((int *)E.bslot, c->d_one_slot, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(&st, E.status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->h_bslot[b] = eff = shadow;
        if (st < 0) return fail(c, MEDGP_ERR_ARG, "batch entry %d: the factorisation in the caller's order failed (status %d)", b, st);
    }
    const bool caller_order = eff >= S || c->h_perm_identity[slot];
    if (alpha) {
        std::vector<double> ha(n);
        HIPCHK(c, hipMemcpy(ha.data(), E.alpha, sizeof(double) * n, hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) alpha[caller_order ? i : perm[i]] = (float)ha[i];
    }
    if (beta) {
        double sc[4];
        HIPCHK(c, hipMemcpy(sc, E.scal, sizeof(sc), hipMemcpyDeviceToHost));
        *beta = (float)sc[1];
    }
    if (linv) {
        const char *hp = nullptr;
        int rc2 = d2h_pinned(c, E.Linv, sizeof(double) * n * ld, &hp);
        if (rc2) return rc2;
        const double *hx = (const double *)hp;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < n; j++)   // device holds U = L^-T: (L^-1)[i][j] = U[j][i]; strict upper zeroed as ref c_inference_exact.cpp:139-143
                linv[(size_t)i * n + j] = (j <= i) ? (float)hx[(size_t)j * ld + i] : 0.0f;
    }
    return MEDGP_OK;
}

// common part of medgp_fit_predict / medgp_fit_predict_batch: nbatch problems x nstar test points each
static int fit_predict_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int nstar,
                            const int32_t *meta2, const float *t2, float *mean, float *var, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !t2 || !mean || !var || nstar < 1 || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    if (c->kidx == MEDGP_KERNEL_LMC_SM && !meta2) return fail(c, MEDGP_ERR_ARG, "meta2 is NULL for the multi-output kernel");
    HIPCHK(c, hipSetDevice(c->device));
    const int ntot = nbatch * nstar;
    std::vector<double> ht2;
    std::vector<int> hm2;
    if ((rc = check_meta2(c, ntot, meta2))) return rc;
    stage_points(c, ntot, meta2, t2, nullptr, ht2, hm2);
    // (no tile table: one workgroup of k_predict per point; its work rows are k* -> v = L^-1 k*, one column per point)
    if ((rc = upload_point_call(c, ntot, ht2, hm2, std::vector<PostTile>(), (size_t)ntot * c->ldn * sizeof(double)))) return rc;
    // patients are used in the caller's order when that differs from the grouped one?  No: mean / var are permutation
    // invariant, the grouped copy serves.
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;   // (the diagonal blocks U_kk live in Linv)
    // factor + z = L^-1 y only (no inverse): k* rides along as one more right-hand side in k_predict
    if ((rc = factor_run(c, nbatch, theta, false, true))) return rc;
    for (const SizeClass &k : c->plan.cls) {   // (behind the join of the classes' chains: one launch per class view)
        Launcher l(c, KID_PREDICT);
        hipLaunchKernelGGL(k_predict, dim3(nstar, k.count), dim3(256), 0, c->stream, class_view(c, c->plan, k), nstar, buf<int>(c, BUF_META2), buf<double>(c, BUF_T2),
                           buf<double>(c, BUF_WORK), buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR));
    }
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair(c, ntot, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), mean, var))) return rc;
    return read_status(c, nbatch, status);
}

int medgp_factor_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, double *const *Lout, double *const *zout,
                       int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if ((rc = set_batch(c, nbatch, slots, true, false))) return rc;       // the CALLER's observation order; size classes; L and z only: no Linv
    if ((rc = factor_run(c, nbatch, theta, false, false))) return rc;
    std::vector<int32_t> st(nbatch, 0);
    if ((rc = read_status(c, nbatch, st.data()))) return rc;
    if (status) for (int b = 0; b < nbatch; b++) status[b] = st[b];
    // every entry's rows of the batch buffers (its size class's view) and leading dimension
    std::vector<MedgpDev> ev(nbatch);
    for (int b = 0; b < nbatch; b++) ev[b] = entry_view(c, b);
    // export: the n x ld leading rows of every successful entry, through the pinned bounce buffer in groups of <= 256 MB
    size_t b0 = 0;
    while (Lout && b0 < (size_t)nbatch) {
        size_t b1 = b0, bytes = 0;
        std::vector<size_t> off;
        while (b1 < (size_t)nbatch) {
            const int n = c->h_n[slots[b1]];
            const size_t need = (st[b1] >= 0 && Lout[b1] && n > 0) ? sizeof(double) * n * ev[b1].ldn : 0;
            if (b1 > b0 && bytes + need > ((size_t)256 << 20)) break;
            off.push_back(bytes); bytes += need; b1++;
        }
        if (bytes > c->bounce_cap) {
            if (c->h_bounce) (void)hipHostFree(c->h_bounce);
            c->h_bounce = nullptr; c->bounce_cap = 0;
            HIPCHK(c, hipHostMalloc((void **)&c->h_bounce, bytes + bytes / 4, hipHostMallocDefault));
            c->bounce_cap = bytes + bytes / 4;
        }
        for (size_t b = b0; b < b1; b++) {
            const int n = c->h_n[slots[b]];
            if (st[b] >= 0 && Lout[b] && n > 0)
                HIPCHK(c, hipMemcpyAsync(c->h_bounce + off[b - b0], ev[b].Kmat, sizeof(double) * n * ev[b].ldn, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t b = b0; b < b1; b++) {
            const int n = c->h_n[slots[b]];
            if (!(st[b] >= 0 && Lout[b] && n > 0)) continue;
            const double *hl = (const double *)(c->h_bounce + off[b - b0]);
            const size_t ld = ev[b].ldn;
            double *Lo = Lout[b];
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) Lo[(size_t)i * n + j] = (j <= i) ? hl[(size_t)i * ld + j] : 0.0;
        }
        b0 = b1;
    }
    if (zout) {
        for (int b = 0; b < nbatch; b++) {
            const int n = c->h_n[slots[b]];
            if (st[b] >= 0 && zout[b] && n > 0)
                HIPCHK(c, hipMemcpyAsync(zout[b], ev[b].z, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return MEDGP_OK;
}

int medgp_factor(medgp_ctx *c, int slot, const double *theta, double *Lout, double *zout, int32_t *status) {
    int32_t s1 = slot;
    double *Lp[1] = {Lout}, *zp[1] = {zout};
    return medgp_factor_batch(c, 1, &s1, theta, Lout ? Lp : nullptr, zout ? zp : nullptr, status);
}

int medgp_pin_route(medgp_ctx *c, int pinned) {
    if (!c) return MEDGP_ERR_ARG;
    c->rules.pin_route = pinned ? 1 : 0;
    return MEDGP_OK;
}

int medgp_last_plan(const medgp_ctx *c, int max_classes, int32_t *count, int32_t *blocks, int32_t *route) {
    if (!c) return MEDGP_ERR_ARG;
    const int nc = (int)c->plan.cls.size();
    for (int i = 0; i < nc && i < max_classes; i++) {
        if (count) count[i] = c->plan.cls[i].count;
        if (blocks) blocks[i] = c->plan.cls[i].nbmax;
        if (route) route[i] = c->plan.cls[i].route;
    }
    return nc;
}

int medgp_fit_predict(medgp_ctx *c, int slot, const double *theta, int nstar, const int32_t *meta2, const float *t2,
                      float *mean, float *var, int32_t *status) {
    int32_t s1 = slot;
    return fit_predict_impl(c, 1, &s1, theta, nstar, meta2, t2, mean, var, status);
}

int medgp_fit_predict_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int32_t *meta2,
                            const float *t2, float *mean, float *var, int32_t *status) {
    return fit_predict_impl(c, nbatch, slots, theta, 1, meta2, t2, mean, var, status);
}

namespace {
void launch_posterior(medgp_ctx *c, const MedgpDev &V, int ntiles, const PostTile *tiles, size_t stride, int with_parts, int parts_lds) {
    const size_t lds = parts_lds ? sizeof(double) * 64 * V.D : 0;
    with_q8(V.Q, [&](auto q) {   // Q > 8: generic component loop
        hipLaunchKernelGGL(k_posterior<decltype(q)::value>, dim3(ntiles), dim3(256), lds, c->stream, V, tiles, buf<int>(c, BUF_META2), buf<double>(c, BUF_T2),
                           buf<double>(c, BUF_WORK), stride, with_parts, parts_lds, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), buf<float>(c, BUF_PARTS));
    });
}

void launch_postcov(medgp_ctx *c, const MedgpDev &V, int npairs, const JointTile *pairs, size_t stride, float *cov) {
    with_q8(V.Q, [&](auto q) {   // Q > 8: generic component loop
        hipLaunchKernelGGL(k_postcov<decltype(q)::value>, dim3(npairs), dim3(256), 0, c->stream, V, buf<JointPat>(c, BUF_PATS), pairs, buf<int>(c, BUF_META2),
                           buf<double>(c, BUF_T2), buf<double>(c, BUF_WORK), stride, buf<double>(c, BUF_C), cov);
    });
}

void launch_forecast(medgp_ctx *c, const MedgpDev &V, int ntiles, const ForeTile *tiles, size_t stride, bool with_lpd, double log2pi) {
    with_q8(V.Q, [&](auto q) {   // Q > 8: generic component loop
        hipLaunchKernelGGL(k_forecast<decltype(q)::value>, dim3(ntiles), dim3(256), 0, c->stream, V, tiles, buf<int>(c, BUF_META2), buf<double>(c, BUF_T2),
                           buf<int>(c, BUF_PREFIX), with_lpd ? buf<double>(c, BUF_Y2) : nullptr, buf<double>(c, BUF_WORK), stride, log2pi,
                           buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), buf<double>(c, BUF_LPD));
    });
}

// the joint outputs of medgp_posterior_joint_batch (null: medgp_posterior_batch)
struct JointReq {
    int nsamp;
    const double *eps;
    float *cov, *samples;
    int32_t *cov_status;
};

// medgp_posterior_batch and medgp_posterior_joint_batch: ONE code path for mean / var (same pipeline run, same k_posterior launches
// per tile: the bits of a point do not depend on the launch chunk).  A joint call cuts its launch chunks at patient boundaries and
// runs k_postcov / k_postfactor / k_postdraw behind k_posterior on each chunk, while the chunk's work rows are resident.
int posterior_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                   const int32_t *meta2, const float *t2, float *mean, float *var, float *parts, int32_t *status, const JointReq *jq) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !offsets || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, !mean || !var, "mean / var");
    if (M < 0) return (int)M;
    const bool want_cov = jq && jq->cov, want_samp = jq && jq->nsamp > 0;
    if (jq) {
        if (jq->nsamp < 0) return fail(c, MEDGP_ERR_ARG, "nsamp = %d", jq->nsamp);
        if (!want_cov && !want_samp) return fail(c, MEDGP_ERR_ARG, "neither cov nor samples asked for (cov == NULL and nsamp == 0)");
        if (want_samp && M > 0 && (!jq->eps || !jq->samples)) return fail(c, MEDGP_ERR_ARG, "eps / samples is NULL with nsamp = %d", jq->nsamp);
        if (want_samp && M * (int64_t)jq->nsamp > (int64_t)INT32_MAX) return fail(c, MEDGP_ERR_ARG, "%lld x %d sample values in one call", (long long)M, jq->nsamp);
    }
    const int D = c->rules.D;
    std::vector<size_t> cov_off(want_cov ? nbatch : 0);   // start of patient b's block in cov (floats)
    if (want_cov) { size_t o = 0; for (int b = 0; b < nbatch; b++) { cov_off[b] = o; const size_t m = (size_t)(offsets[b + 1] - offsets[b]); o += m * m; } }
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, nullptr, ht2, hm2);
    HIPCHK(c, hipSetDevice(c->device));
    // the parts, like mean and var, are invariant under a permutation of the training observations: the grouped copy serves
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const bool with_parts = parts != nullptr;
    const int parts_lds = D <= POST_PARTS_LDS_MAX_D;
    JointTables T;
    const size_t extra = (with_parts && !parts_lds) ? (size_t)D * 64 : 0;   // doubles per tile beyond its 64 work rows
    if (!jq) build_point_tiles(table_classes(c->plan), c->plan.order.data(), offsets, nullptr, extra, c->posterior_budget, T);
    else {
        TableError e;
        if (!build_joint_chunks(table_classes(c->plan), c->plan.order.data(), offsets, extra, want_cov, c->posterior_budget, T, e))
            return fail(c, MEDGP_ERR_CAPACITY, "patient %d: the joint posterior of %lld points on %d observations needs %zu MB at once, the budget is %zu MB (MEDGP_POSTERIOR_BUDGET_GB)",
                        e.b, e.m, c->plan.en[e.entry], e.need >> 20, c->posterior_budget >> 20);
    }
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if (with_parts && (rc = buf_ensure(c, BUF_PARTS, (size_t)std::max<int64_t>(M, 1) * D * sizeof(float)))) return rc;
    if (jq) {
        if ((rc = buf_ensure(c, BUF_CSTAT, sizeof(int) * nbatch))) return rc;
        HIPCHK(c, hipMemsetAsync(buf<int>(c, BUF_CSTAT), 0, sizeof(int) * nbatch, c->stream));
    }
    if (jq && !T.pats.empty()) {
        if ((rc = upload_table(c, BUF_PATS, T.pats))) return rc;
        if ((rc = upload_table(c, BUF_PAIRS, T.pairs))) return rc;
        if ((rc = upload_table(c, BUF_BLKS, T.blks))) return rc;
        if ((rc = buf_ensure(c, BUF_C, T.c_need))) return rc;
        if (want_cov && (rc = buf_ensure(c, BUF_COV, T.cov_need))) return rc;
        if (want_samp) {
            const size_t ns = (size_t)M * jq->nsamp;
            if ((rc = buf_ensure(c, BUF_EPS, ns * sizeof(double)))) return rc;
            if ((rc = buf_ensure(c, BUF_SAMP, ns * sizeof(float)))) return rc;
            HIPCHK(c, hipMemcpyAsync(buf<double>(c, BUF_EPS), jq->eps, ns * sizeof(double), hipMemcpyHostToDevice, c->stream));
        }
    }
    // factor + z = L^-1 y + the diagonal-block inverses U_kk (no inverse): the ONE pipeline run of the call
    if ((rc = factor_run(c, nbatch, theta, false, true))) return rc;
    if (with_parts && M > 0)
        for (const SizeClass &k : c->plan.cls) {   // (behind the join of the classes' chains)
            Launcher l(c, KID_ALPHA);
            hipLaunchKernelGGL(k_alpha, dim3(k.count), dim3(256), 0, c->stream, class_view(c, c->plan, k));
        }
    const JointPat *d_pats = buf<JointPat>(c, BUF_PATS);
    double *d_C = buf<double>(c, BUF_C);
    int *d_cstat = buf<int>(c, BUF_CSTAT);
    for (const TileChunk &ch : T.chunks) {   // chunks reuse the work rows in stream order
        Launcher l(c, KID_POSTERIOR);
        const MedgpDev V = class_view(c, c->plan, c->plan.cls[ch.cls]);
        launch_posterior(c, V, ch.nt, buf<PostTile>(c, BUF_TILES) + ch.t0, ch.stride, with_parts ? 1 : 0, parts_lds);
        if (!jq) continue;
        l.finish();
        {
            Launcher lc(c, KID_POSTCOV);
            launch_postcov(c, V, ch.npair, buf<JointTile>(c, BUF_PAIRS) + ch.pair0, ch.stride, want_cov ? buf<float>(c, BUF_COV) : nullptr);
        }
        if (want_samp) {   // (a covariance-only call factors nothing)
            {
                Launcher lf(c, KID_POSTFACTOR);
                hipLaunchKernelGGL(k_postfactor, dim3(ch.npat), dim3(256), 0, c->stream, V, d_pats + ch.pat0, d_C, d_cstat);
            }
            Launcher ld(c, KID_POSTDRAW);
            hipLaunchKernelGGL(k_postdraw, dim3(ch.nblk), dim3(256), 0, c->stream, V, d_pats, buf<JointTile>(c, BUF_BLKS) + ch.blk0, buf<double>(c, BUF_WORK), ch.stride,
                               d_C, d_cstat, buf<double>(c, BUF_EPS), jq->nsamp, buf<float>(c, BUF_SAMP));
        }
        if (want_cov)   // the chunk's blocks go home before the next chunk reuses the buffer (stream order)
            for (int i = ch.pat0; i < ch.pat0 + ch.npat; i++) {
                const JointPat &P = T.pats[i];
                HIPCHK(c, hipMemcpyAsync(jq->cov + cov_off[P.b], buf<float>(c, BUF_COV) + P.voff, sizeof(float) * (size_t)P.m * P.m, hipMemcpyDeviceToHost, c->stream));
            }
    }
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair(c, M, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), mean, var))) return rc;
    if (M > 0) {
        if (with_parts) HIPCHK(c, hipMemcpyAsync(parts, buf<float>(c, BUF_PARTS), sizeof(float) * M * D, hipMemcpyDeviceToHost, c->stream));
        if (want_samp) HIPCHK(c, hipMemcpyAsync(jq->samples, buf<float>(c, BUF_SAMP), sizeof(float) * (size_t)M * jq->nsamp, hipMemcpyDeviceToHost, c->stream));
    }
    std::vector<int> st, cst(nbatch, 0);
    if (jq) HIPCHK(c, hipMemcpyAsync(cst.data(), d_cstat, sizeof(int) * nbatch, hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_status(c, nbatch, status, jq ? &st : nullptr))) return rc;
    if (jq && jq->cov_status)   // (caller order on the device; a patient without a factor has no C either)
        for (int i = 0; i < nbatch; i++) { const int b = c->plan.order[i]; jq->cov_status[b] = (st[i] < 0 || cst[b] < 0) ? -1 : 0; }
    return MEDGP_OK;
}

// medgp_forecast_batch (kernels_forecast.h): the posterior call's pipeline run on the CALLER-order copies, then k_forecast over tiles
// of points sorted by prefix inside each patient (a tile's panel count follows its largest prefix).  The device sees the points in
// the sorted order; the outputs are scattered back on the host.  A point's bits do not depend on its tile, so the sort is invisible.
int forecast_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets, const int32_t *meta2,
                  const float *t2, const int32_t *prefix, const float *y2, float *mean, float *var, double *lpd, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !offsets || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    if ((y2 == nullptr) != (lpd == nullptr)) return fail(c, MEDGP_ERR_ARG, "y2 and lpd must both be given or both be NULL");
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, !mean || !var, "mean / var");
    if (M < 0) return (int)M;
    // the device order of the points: inside each patient stably sorted by prefix (src[k] = the caller's index of device point k)
    std::vector<int64_t> src(M);
    std::vector<int> hpf(M);
    for (int b = 0; b < nbatch; b++) {
        const int n = c->h_n[slots[b]];
        for (int64_t j = offsets[b]; j < offsets[b + 1]; j++) {
            if (prefix && (prefix[j] < 0 || prefix[j] > n))
                return fail(c, MEDGP_ERR_ARG, "prefix[%lld] = %d outside [0, %d] (patient %d)", (long long)j, prefix[j], n, b);
            src[j] = j;
        }
        if (prefix)
            std::stable_sort(src.begin() + offsets[b], src.begin() + offsets[b + 1], [&](int64_t a, int64_t z) { return prefix[a] < prefix[z]; });
        for (int64_t k = offsets[b]; k < offsets[b + 1]; k++) hpf[k] = prefix ? prefix[src[k]] : n;
    }
    std::vector<double> ht2, hy2(y2 ? M : 0);
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, src.data(), ht2, hm2);
    for (int64_t k = 0; y2 && k < M; k++) hy2[k] = (double)y2[src[k]];
    HIPCHK(c, hipSetDevice(c->device));
    // "the first p observations" is the caller's order: a patient not uploaded grouped by output is factored on its caller-order copy
    if ((rc = set_batch(c, nbatch, slots, true, true))) return rc;
    // tile table per size class and launch chunks within the budget, as the posterior call's -- and in its buffers
    static_assert(sizeof(ForeTile) == sizeof(PostTile), "the forecast tiles travel in the posterior call's tile buffer");
    PointTables<ForeTile> T;
    build_point_tiles(table_classes(c->plan), c->plan.order.data(), offsets, hpf.data(), 0, c->posterior_budget, T);
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = upload_table(c, BUF_PREFIX, hpf))) return rc;
    if (y2 && (rc = upload_table(c, BUF_Y2, hy2))) return rc;
    if (y2 && (rc = buf_ensure(c, BUF_LPD, (size_t)std::max<int64_t>(M, 1) * sizeof(double)))) return rc;
    // factor + z = L^-1 y + the diagonal-block inverses U_kk (no inverse): the ONE pipeline run of the call
    if ((rc = factor_run(c, nbatch, theta, false, true))) return rc;
    const double log2pi = std::log(2.0 * c->pi);
    for (const TileChunk &ch : T.chunks) {   // chunks reuse the work rows in stream order
        Launcher l(c, KID_FORECAST);
        launch_forecast(c, class_view(c, c->plan, c->plan.cls[ch.cls]), ch.nt, buf<ForeTile>(c, BUF_TILES) + ch.t0, ch.stride, y2 != nullptr, log2pi);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<float> hmv;
    std::vector<double> hlpd(y2 ? M : 0);
    if ((rc = download_pair(c, M, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), mean, var, &hmv))) return rc;
    if (M > 0 && y2) HIPCHK(c, hipMemcpyAsync(hlpd.data(), buf<double>(c, BUF_LPD), sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_status(c, nbatch, status))) return rc;
    unsort_pair(hmv, src.data(), mean, var);   // sorted order -> the caller's
    for (int64_t k = 0; y2 && k < M; k++) lpd[src[k]] = hlpd[k];
    return MEDGP_OK;
}

// medgp_trend_batch (kernels_trend.h): the posterior call's pipeline run, then k_trend over tiles of TREND_TW points whose 64 columns
// carry the value and the slope column of every point through the same panel loop.  Launch chunks within the posterior budget.
int trend_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets, const int32_t *meta2,
               const float *t2, float *mean, float *var, float *dmean, float *dvar, float *cross, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !offsets || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    if (!dmean || !dvar) return fail(c, MEDGP_ERR_ARG, "dmean / dvar is NULL");
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, !mean || !var, "mean / var");
    if (M < 0) return (int)M;
    const size_t Mz = (size_t)std::max<int64_t>(M, 1);
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, nullptr, ht2, hm2);
    HIPCHK(c, hipSetDevice(c->device));
    // the five outputs are invariant under a permutation of the training observations: the grouped copy serves, as for the posterior
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    PointTables<PostTile> T;
    build_trend_tiles(table_classes(c->plan), c->plan.order.data(), offsets, c->posterior_budget, T);
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = buf_ensure(c, BUF_SLOPE, 3 * Mz * sizeof(float)))) return rc;
    // factor + z = L^-1 y + the diagonal-block inverses U_kk (no inverse): the ONE pipeline run of the call
    if ((rc = factor_run(c, nbatch, theta, false, true))) return rc;
    float *d_dmean = buf<float>(c, BUF_SLOPE), *d_dvar = d_dmean + Mz, *d_cross = d_dvar + Mz;
    for (const TileChunk &ch : T.chunks) {   // chunks reuse the work rows in stream order
        Launcher l(c, KID_TREND);
        const MedgpDev V = class_view(c, c->plan, c->plan.cls[ch.cls]);
        with_q8(V.Q, [&](auto q) {   // Q > 8: generic component loop
            hipLaunchKernelGGL(k_trend<decltype(q)::value>, dim3(ch.nt), dim3(256), 0, c->stream, V, buf<PostTile>(c, BUF_TILES) + ch.t0, buf<int>(c, BUF_META2),
                               buf<double>(c, BUF_T2), buf<double>(c, BUF_WORK), ch.stride, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), d_dmean, d_dvar,
                               cross ? d_cross : nullptr);
        });
    }
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair(c, M, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), mean, var))) return rc;
    if ((rc = download_pair<float>(c, M, d_dmean, d_dvar, dmean, dvar))) return rc;
    if (M > 0 && cross) HIPCHK(c, hipMemcpyAsync(cross, d_cross, sizeof(float) * M, hipMemcpyDeviceToHost, c->stream));
    return read_status(c, nbatch, status);
}

// medgp_components_batch (kernels_components.h): the posterior call's pipeline run, then k_components over tiles of 64 / Q points whose
// 64 columns are the Q component columns of every point.  Launch chunks within the posterior budget; the launches are accounted under
// the profile entry of k_posterior (the profile table keeps its names).
int components_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets, const int32_t *meta2,
                    const float *t2, float *cmean, float *cvar, float *ccov, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !offsets || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    if (!cmean || !cvar) return fail(c, MEDGP_ERR_ARG, "cmean / cvar is NULL");
    const int Q = c->rules.Q;
    if (Q > 64) return fail(c, MEDGP_ERR_ARG, "medgp_components_batch supports Q <= 64 (Q = %d): the component columns of a point share one 64-column tile", Q);
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, false, "cmean / cvar");   // (cmean / cvar: checked above)
    if (M < 0) return (int)M;
    const size_t MQ = (size_t)std::max<int64_t>(M, 1) * Q;
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, nullptr, ht2, hm2);
    HIPCHK(c, hipSetDevice(c->device));
    // the outputs are invariant under a permutation of the training observations: the grouped copy serves, as for the posterior
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    PointTables<PostTile> T;
    build_components_tiles(table_classes(c->plan), c->plan.order.data(), offsets, Q, ccov != nullptr, c->posterior_budget, T);
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = buf_ensure(c, BUF_COMP, MQ * (2 + (ccov ? (size_t)Q : 0)) * sizeof(float)))) return rc;
    // factor + z = L^-1 y + the diagonal-block inverses U_kk (no inverse): the ONE pipeline run of the call
    if ((rc = factor_run(c, nbatch, theta, false, true))) return rc;
    float *d_cmean = buf<float>(c, BUF_COMP), *d_cvar = d_cmean + MQ, *d_ccov = d_cvar + MQ;
    for (const TileChunk &ch : T.chunks) {   // chunks reuse the work rows in stream order
        Launcher l(c, KID_POSTERIOR);
        hipLaunchKernelGGL(k_components, dim3(ch.nt), dim3(256), 0, c->stream, class_view(c, c->plan, c->plan.cls[ch.cls]), buf<PostTile>(c, BUF_TILES) + ch.t0,
                           buf<int>(c, BUF_META2), buf<double>(c, BUF_T2), buf<double>(c, BUF_WORK), ch.stride, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR),
                           d_cmean, d_cvar, ccov ? d_ccov : nullptr);
    }
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair<float>(c, M * Q, d_cmean, d_cvar, cmean, cvar))) return rc;
    if (M > 0 && ccov) HIPCHK(c, hipMemcpyAsync(ccov, d_ccov, sizeof(float) * M * Q * Q, hipMemcpyDeviceToHost, c->stream));
    return read_status(c, nbatch, status);
}

// medgp_functional_batch (kernels_functional.h): the posterior call's pipeline run, then per size class k_functional_prep (the term
// tables and the prior variances, once per call; accounted under the profile entry of k_prep) and per launch chunk k_functional over
// tiles of 64 functionals, one solve column each; those launches are accounted under the profile entry of k_posterior (the profile
// table keeps its names).  The tile table indexes functionals in the caller's numbering: nothing is scattered.
// medgp_functional_joint_batch (joint; kernels_functional_joint.h) is the SAME code path for fmean / fvar (same pipeline run, same
// k_functional_prep and k_functional launches per tile: the bits of a functional do not depend on the launch chunk).  It cuts its
// launch chunks at patient boundaries and runs k_funccov behind k_functional on each chunk, while the chunk's work rows are resident;
// those launches are accounted under the profile entry of k_postcov.
int functional_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *foffsets, const int64_t *toffsets,
                    const int32_t *meta2, const float *t2, const double *weight, float *fmean, float *fvar, bool joint, float *fcov,
                    int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    if (!fmean || !fvar) return fail(c, MEDGP_ERR_ARG, "fmean / fvar is NULL");
    if (joint && !fcov) return fail(c, MEDGP_ERR_ARG, "fcov is NULL");
    if (!foffsets || !toffsets || !t2 || !weight) return fail(c, MEDGP_ERR_ARG, "foffsets / toffsets / t2 / weight is NULL");
    if (c->kidx == MEDGP_KERNEL_LMC_SM && !meta2) return fail(c, MEDGP_ERR_ARG, "meta2 is NULL for the multi-output kernel");
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    FunctionalCsr S;
    switch (check_functional_csr(foffsets, toffsets, nbatch, S)) {
    case FUNC_CSR_OK: break;
    case FUNC_CSR_FIRST: return fail(c, MEDGP_ERR_ARG, "foffsets[0] = %lld, expected 0", (long long)foffsets[0]);
    case FUNC_CSR_DECREASE: return fail(c, MEDGP_ERR_ARG, "foffsets decrease at %lld", (long long)S.at);
    case FUNC_CSR_COUNT: return fail(c, MEDGP_ERR_ARG, "%lld functionals in one call (at most %lld)", (long long)foffsets[nbatch], (long long)FUNC_MAX_FUNCTIONALS);
    case FUNC_CSR_TERM_FIRST: return fail(c, MEDGP_ERR_ARG, "toffsets[0] = %lld, expected 0", (long long)toffsets[0]);
    case FUNC_CSR_TERM_DECREASE: return fail(c, MEDGP_ERR_ARG, "toffsets decrease at %lld", (long long)S.at);
    case FUNC_CSR_TERM_COUNT: return fail(c, MEDGP_ERR_ARG, "more than %lld terms in one call (functional %lld)", (long long)FUNC_MAX_TERMS, (long long)S.at);
    default: return fail(c, MEDGP_ERR_ARG, "foffsets / toffsets is NULL");
    }
    const int64_t F = S.F, Tn = S.T;
    const size_t Fz = (size_t)std::max<int64_t>(F, 1), Tz = (size_t)std::max<int64_t>(Tn, 1), Q = (size_t)c->rules.Q;
    std::vector<double> ht2;
    std::vector<int> hm2;
    if ((rc = check_meta2(c, Tn, meta2))) return rc;   // (the terms' covariates are range-checked as the posterior call's points)
    stage_points(c, Tn, meta2, t2, nullptr, ht2, hm2);
    HIPCHK(c, hipSetDevice(c->device));
    // the outputs are invariant under a permutation of the training observations: the grouped copy serves, as for the posterior
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const std::vector<TableClass> cls = table_classes(c->plan);
    JointTables T;
    if (!joint) build_functional_tiles(cls, c->plan.order.data(), foffsets, c->posterior_budget, T);
    else {
        TableError e;
        if (!build_functional_joint_chunks(cls, c->plan.order.data(), foffsets, c->posterior_budget, T, e))
            return fail(c, MEDGP_ERR_CAPACITY, "patient %d: the joint posterior of %lld functionals on %d observations needs %zu MB at once, the budget is %zu MB (MEDGP_POSTERIOR_BUDGET_GB)",
                        e.b, e.m, c->plan.en[e.entry], e.need >> 20, c->posterior_budget >> 20);
    }
    std::vector<size_t> cov_off(joint ? nbatch : 0);   // start of patient b's block in fcov (floats)
    if (joint) { size_t o = 0; for (int b = 0; b < nbatch; b++) { cov_off[b] = o; const size_t Fb = (size_t)(foffsets[b + 1] - foffsets[b]); o += Fb * Fb; } }
    if ((rc = upload_point_call(c, Tn, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = buf_ensure(c, BUF_MEAN, Fz * sizeof(float)))) return rc;   // (per functional, not per term)
    if ((rc = buf_ensure(c, BUF_VAR, Fz * sizeof(float)))) return rc;
    if ((rc = buf_ensure(c, BUF_FUNC_D, (2 * Tz + Fz + 2 * Tz * Q) * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FUNC_I, (Fz + 1 + Tz) * sizeof(int)))) return rc;
    double *d_w = buf<double>(c, BUF_FUNC_D), *d_rsum = d_w + Tz, *d_qg = d_rsum + Tz, *d_cos = d_qg + Fz, *d_sin = d_cos + Tz * Q;
    int *d_toff = buf<int>(c, BUF_FUNC_I), *d_fun = d_toff + Fz + 1;
    HIPCHK(c, hipMemcpyAsync(d_toff, S.toff.data(), sizeof(int) * (F + 1), hipMemcpyHostToDevice, c->stream));
    if (Tn > 0) {
        HIPCHK(c, hipMemcpyAsync(d_w, weight, sizeof(double) * Tn, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_fun, S.fun.data(), sizeof(int) * Tn, hipMemcpyHostToDevice, c->stream));
    }
    if (joint && !T.pats.empty()) {
        if ((rc = upload_table(c, BUF_PATS, T.pats))) return rc;
        if ((rc = upload_table(c, BUF_PAIRS, T.pairs))) return rc;
        if ((rc = buf_ensure(c, BUF_COV, T.cov_need))) return rc;
    }
    // factor + z = L^-1 y + the diagonal-block inverses U_kk (no inverse): the ONE pipeline run of the call
    if ((rc = factor_run(c, nbatch, theta, false, true))) return rc;
    const FuncTerms ft{d_toff, d_fun, buf<int>(c, BUF_META2), buf<double>(c, BUF_T2), d_w, d_cos, d_sin, d_rsum, d_qg};
    for (size_t i = 0, k = 0; i < T.chunks.size(); i = k) {   // the chunks of a class are consecutive, and so are their tiles
        int nt = 0;
        for (k = i; k < T.chunks.size() && T.chunks[k].cls == T.chunks[i].cls; k++) nt += T.chunks[k].nt;
        Launcher l(c, KID_PREP);
        hipLaunchKernelGGL(k_functional_prep, dim3(nt), dim3(256), 0, c->stream, class_view(c, c->plan, c->plan.cls[T.chunks[i].cls]),
                           buf<PostTile>(c, BUF_TILES) + T.chunks[i].t0, ft);
    }
    for (const TileChunk &ch : T.chunks) {   // chunks reuse the work rows in stream order
        Launcher l(c, KID_POSTERIOR);
        const MedgpDev V = class_view(c, c->plan, c->plan.cls[ch.cls]);
        hipLaunchKernelGGL(k_functional, dim3(ch.nt), dim3(256), 0, c->stream, V, buf<PostTile>(c, BUF_TILES) + ch.t0,
                           ft, buf<double>(c, BUF_WORK), ch.stride, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR));
        if (!joint) continue;
        l.finish();
        {
            Launcher lc(c, KID_POSTCOV);
            hipLaunchKernelGGL(k_funccov, dim3(ch.npair), dim3(256), 0, c->stream, V, buf<JointPat>(c, BUF_PATS), buf<JointTile>(c, BUF_PAIRS) + ch.pair0, ft,
                               buf<double>(c, BUF_WORK), ch.stride, buf<float>(c, BUF_VAR), buf<float>(c, BUF_COV));
        }
        for (int i = ch.pat0; i < ch.pat0 + ch.npat; i++) {   // the chunk's blocks go home before the next chunk reuses the buffer (stream order)
            const JointPat &P = T.pats[i];
            HIPCHK(c, hipMemcpyAsync(fcov + cov_off[P.b], buf<float>(c, BUF_COV) + P.voff, sizeof(float) * (size_t)P.m * P.m, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair(c, F, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), fmean, fvar))) return rc;
    return read_status(c, nbatch, status);
}
}  // namespace

int medgp_functional_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *foffsets,
                           const int64_t *toffsets, const int32_t *meta2, const float *t2, const double *weight, float *fmean,
                           float *fvar, int32_t *status) {
    return functional_impl(c, nbatch, slots, theta, foffsets, toffsets, meta2, t2, weight, fmean, fvar, false, nullptr, status);
}

int medgp_functional_joint_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *foffsets,
                                 const int64_t *toffsets, const int32_t *meta2, const float *t2, const double *weight, float *fmean,
                                 float *fvar, float *fcov, int32_t *status) {
    return functional_impl(c, nbatch, slots, theta, foffsets, toffsets, meta2, t2, weight, fmean, fvar, true, fcov, status);
}

int medgp_components_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                           const int32_t *meta2, const float *t2, float *cmean, float *cvar, float *ccov, int32_t *status) {
    return components_impl(c, nbatch, slots, theta, offsets, meta2, t2, cmean, cvar, ccov, status);
}

int medgp_trend_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                      const int32_t *meta2, const float *t2, float *mean, float *var, float *dmean, float *dvar, float *cross,
                      int32_t *status) {
    return trend_impl(c, nbatch, slots, theta, offsets, meta2, t2, mean, var, dmean, dvar, cross, status);
}

int medgp_posterior_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                          const int32_t *meta2, const float *t2, float *mean, float *var, float *parts, int32_t *status) {
    return posterior_impl(c, nbatch, slots, theta, offsets, meta2, t2, mean, var, parts, status, nullptr);
}

int medgp_posterior_joint_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                                const int32_t *meta2, const float *t2, int nsamp, const double *eps, float *mean, float *var,
                                float *cov, float *samples, int32_t *status, int32_t *cov_status) {
    const JointReq jq{nsamp, eps, cov, samples, cov_status};
    return posterior_impl(c, nbatch, slots, theta, offsets, meta2, t2, mean, var, nullptr, status, &jq);
}

int medgp_forecast_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                         const int32_t *meta2, const float *t2, const int32_t *prefix, const float *y2,
                         float *mean, float *var, double *lpd, int32_t *status) {
    return forecast_impl(c, nbatch, slots, theta, offsets, meta2, t2, prefix, y2, mean, var, lpd, status);
}

// Leave-one-out / leave-group-out predictions of the training observations (kernels_loo.h).  ONE pipeline run in the grouped order
// (the outputs are permutation-equivariant: the caller's group ids are mapped through h_perm and the results scattered back), then
// per size class k_loo_diag over its singleton groups and, per launch chunk of larger groups whose blocks fit the posterior budget,
// k_loo_gram / k_postfactor / k_loo_solve.  Singletons never get a block.  The outputs are filled with NaN on the device first: what no
// kernel writes (observations never held out, failed patients, failed groups) stays NaN.
int medgp_loo_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int32_t *group, const int32_t *ngroups,
                    float *mean, float *var, double *lpd, double *total, int32_t *status, int32_t *group_status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    if (!mean && !var && !lpd && !total) return fail(c, MEDGP_ERR_ARG, "none of mean, var, lpd and total asked for");
    if (group && !ngroups) return fail(c, MEDGP_ERR_ARG, "ngroups is NULL with group ids");
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    std::vector<int64_t> ooff(nbatch + 1, 0), goff(nbatch + 1, 0);   // first observation / first group of patient b in the call
    for (int b = 0; b < nbatch; b++) {
        if (group && ngroups[b] < 0) return fail(c, MEDGP_ERR_ARG, "ngroups[%d] = %d", b, ngroups[b]);
        ooff[b + 1] = ooff[b] + c->h_n[slots[b]];
        goff[b + 1] = goff[b] + (group ? ngroups[b] : c->h_n[slots[b]]);
    }
    const int64_t NO = ooff[nbatch], NG = goff[nbatch];
    if (NO > (int64_t)INT32_MAX || NG > (int64_t)INT32_MAX) return fail(c, MEDGP_ERR_ARG, "%lld observations in %lld groups in one call", (long long)NO, (long long)NG);
    if (group)
        for (int b = 0; b < nbatch; b++)
            for (int64_t i = ooff[b]; i < ooff[b + 1]; i++)
                if (group[i] < -1 || group[i] >= ngroups[b])
                    return fail(c, MEDGP_ERR_ARG, "group[%lld] = %d outside [-1, %d) (patient %d)", (long long)i, group[i], ngroups[b], b);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const bool want_lpd = lpd || total;
    std::vector<const int *> perm(nbatch);   // internal row -> caller observation (null: the patient was uploaded grouped)
    for (int b = 0; b < nbatch; b++) perm[b] = c->h_perm_identity[slots[b]] ? nullptr : c->h_perm[slots[b]].data();
    LooTables T;
    TableError e;
    if (!build_loo_tables(table_classes(c->plan), c->plan.order.data(), c->plan.en.data(), ooff.data(), goff.data(), nbatch, group, perm.data(),
                          var != nullptr, mean || want_lpd, c->posterior_budget, T, e))
        return fail(c, MEDGP_ERR_CAPACITY, "patient %d: group %d of %d observations needs %zu MB at once, the budget is %zu MB (MEDGP_POSTERIOR_BUDGET_GB)",
                    e.b, e.gid, (int)e.m, e.need >> 20, c->posterior_budget >> 20);
    const size_t NOz = (size_t)std::max<int64_t>(NO, 1), NGz = (size_t)std::max<int64_t>(NG, 1);
    if ((rc = buf_ensure(c, BUF_MEAN, NOz * sizeof(float)))) return rc;
    if ((rc = buf_ensure(c, BUF_VAR, NOz * sizeof(float)))) return rc;
    if ((rc = buf_ensure(c, BUF_LPD, NGz * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_CSTAT, NGz * sizeof(int)))) return rc;
    if ((rc = buf_ensure(c, BUF_C, T.blk_need))) return rc;
    float *d_mean = buf<float>(c, BUF_MEAN), *d_var = buf<float>(c, BUF_VAR);
    double *d_lpd = buf<double>(c, BUF_LPD), *d_blocks = buf<double>(c, BUF_C);
    int *d_gstat = buf<int>(c, BUF_CSTAT);
    HIPCHK(c, hipMemsetAsync(d_mean, 0xFF, NOz * sizeof(float), c->stream));   // all ones: NaN, float and double
    HIPCHK(c, hipMemsetAsync(d_var, 0xFF, NOz * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(d_lpd, 0xFF, NGz * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(d_gstat, 0, NGz * sizeof(int), c->stream));
    if ((rc = upload_table(c, BUF_SINGLES, T.singles))) return rc;
    if ((rc = upload_table(c, BUF_ROWS, T.rows))) return rc;
    if ((rc = upload_table(c, BUF_PATS, T.groups))) return rc;
    if ((rc = upload_table(c, BUF_PAIRS, T.pairs))) return rc;
    if ((rc = upload_table(c, BUF_BLKS, T.jobs))) return rc;
    const LooSingle *d_singles = buf<LooSingle>(c, BUF_SINGLES);
    const LooRow *d_rows = buf<LooRow>(c, BUF_ROWS);
    const JointPat *d_groups = buf<JointPat>(c, BUF_PATS);
    const JointTile *d_pairs = buf<JointTile>(c, BUF_PAIRS), *d_jobs = buf<JointTile>(c, BUF_BLKS);
    // factor, U = L^-T and alpha = K^-1 y of every entry: the ONE pipeline run of the call (medgp_get_factor is valid afterwards)
    if ((rc = factor_run(c, nbatch, theta, true, false))) return rc;
    const double log2pi = std::log(2.0 * c->pi);
    for (const LooClassSingles &s : T.csing) {
        if (s.ns == 0) continue;
        Launcher l(c, KID_LOO_DIAG);
        hipLaunchKernelGGL(k_loo_diag, dim3((s.ns + 3) / 4), dim3(256), 0, c->stream, class_view(c, c->plan, c->plan.cls[s.cls]), d_singles + s.s0, s.ns, log2pi,
                           mean ? d_mean : nullptr, var ? d_var : nullptr, want_lpd ? d_lpd : nullptr);
    }
    for (const LooChunk &ch : T.chunks) {   // chunks reuse the blocks in stream order
        const MedgpDev V = class_view(c, c->plan, c->plan.cls[ch.cls]);
        {
            Launcher l(c, KID_LOO_GRAM);
            hipLaunchKernelGGL(k_loo_gram, dim3(ch.npair), dim3(256), 0, c->stream, V, d_groups, d_pairs + ch.pair0, d_rows, d_blocks);
        }
        {
            Launcher l(c, KID_POSTFACTOR);
            hipLaunchKernelGGL(k_postfactor, dim3(ch.ng), dim3(256), 0, c->stream, V, d_groups + ch.g0, d_blocks, d_gstat);
        }
        if (ch.njob > 0) {
            Launcher l(c, KID_LOO_SOLVE);
            hipLaunchKernelGGL(k_loo_solve, dim3(ch.njob), dim3(256), 0, c->stream, V, d_groups, d_jobs + ch.job0, d_rows, d_blocks, d_gstat, log2pi,
                               mean ? d_mean : nullptr, var ? d_var : nullptr, want_lpd ? d_lpd : nullptr);
        }
    }
    HIPCHK(c, hipGetLastError());
    std::vector<double> hl(lpd ? 0 : (want_lpd ? (size_t)NG : 0));
    double *lp = lpd ? lpd : hl.data();
    std::vector<int> st, gst((size_t)NG, 0);
    if (mean && NO > 0) HIPCHK(c, hipMemcpyAsync(mean, d_mean, sizeof(float) * NO, hipMemcpyDeviceToHost, c->stream));
    if (var && NO > 0) HIPCHK(c, hipMemcpyAsync(var, d_var, sizeof(float) * NO, hipMemcpyDeviceToHost, c->stream));
    if (want_lpd && NG > 0) HIPCHK(c, hipMemcpyAsync(lp, d_lpd, sizeof(double) * NG, hipMemcpyDeviceToHost, c->stream));
    if (NG > 0) HIPCHK(c, hipMemcpyAsync(gst.data(), d_gstat, sizeof(int) * NG, hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_status(c, nbatch, status, &st))) return rc;
    for (int i = 0; i < nbatch; i++) {
        const int b = c->plan.order[i];
        const bool ok = st[i] >= 0;
        double sum = 0.0;
        for (int64_t g = goff[b]; g < goff[b + 1]; g++) {
            if (group_status) group_status[g] = (!ok || gst[g] < 0) ? -1 : 0;
            if (!want_lpd) continue;
            if (ok && T.gsize[g] == 0) lp[g] = 0.0;   // an empty group
            sum += lp[g];                              // (group-id order)
        }
        if (total) total[b] = ok ? sum : (double)NAN;
    }
    return MEDGP_OK;
}

// The negative LOO log pseudo-likelihood and its gradient (kernels_loo_grad.h).  ONE pipeline run in the grouped order (as
// medgp_loo_batch: factor, U = L^-T, alpha), then per size class, in stream order: k_loo_kinv (P = U U^T into the dead Kmat block),
// k_loo_vec (u, s, log p; then v = P u and J -> scal[2]), k_loo_wgrad (W_loo tiles -> slab, wdiag), and finish_objective_class
// (k_slabsum, k_epilogue).  flag_grad = 0 stops after the first pass of k_loo_vec.
int medgp_loo_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int flag_grad, double *obj, double *grad,
                   int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !obj) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (flag_grad & ~1) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    if (flag_grad && !grad) return fail(c, MEDGP_ERR_ARG, "grad is NULL with flag_grad set");
    int rc;
    if ((rc = check_q16(c, "medgp_loo_grad", kWhyKinv))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = buf_ensure(c, BUF_GVEC, 4 * P.need_vec * sizeof(double)))) return rc;
    double *gvec = buf<double>(c, BUF_GVEC);
    if ((rc = wait_lane0_staging(c))) return rc;
    if ((rc = factor_run_templated(c, nbatch, theta))) return rc;
    const double log2pi = std::log(2.0 * c->pi);
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        double *vec = gvec + 4 * k.off_vec;
        const int nb = k.count, nt64 = k.nbmax;
        { Launcher l(c, KID_LOO_VEC); hipLaunchKernelGGL(k_loo_vec, dim3(4 * nt64, nb), dim3(256), 0, c->stream, V, vec, 0, log2pi); }
        if (!flag_grad) {
            Launcher l(c, KID_LOO_VEC);
            hipLaunchKernelGGL(k_loo_vec, dim3(1, nb), dim3(256), 0, c->stream, V, vec, 2, log2pi);
        } else {
            const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, nb, nt64);
            launch_kinv(c, P, k, V);
            { Launcher l(c, KID_LOO_VEC); hipLaunchKernelGGL(k_loo_vec, dim3(4 * nt64, nb), dim3(256), 0, c->stream, V, vec, 1, log2pi); }
            launch_tiles(c, KID_LOO_WGRAD, V.Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
                hipLaunchKernelGGL((k_loo_wgrad<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, V, vec, nb, wg.wg_tiles, wg.nbp);
            });
        }
        finish_objective_class(c, V, nb, flag_grad);
    }
    HIPCHK(c, hipGetLastError());
    return download_objective(c, nbatch, flag_grad, obj, grad, status);
}

// The negative leave-group-out log pseudo-likelihood and its gradient (kernels_lgo_grad.h).  ONE pipeline run in the grouped order (as
// medgp_loo_batch: the caller's group ids go through h_perm), then per size class, in stream order: k_loo_vec mode 0 and k_lgo_mask (the
// singleton groups: u, s, lpd), for a gradient k_loo_kinv (P into the dead Kmat block) and k_lgo_prep (Tt = P diag(s)); per launch
// chunk of the class's larger groups k_loo_gram / k_postfactor / k_loo_solve (R, w, lpd_g: medgp_loo_batch's kernels and bits) and, for
// a gradient, k_lgo_inv (R^-1), k_lgo_s (S_g, r_g) and k_lgo_t (the group's columns of Tt) -- a chunk is finished before the next one
// reuses the blocks; then k_loo_vec mode 1 (v = P r), k_lgo_obj (J -> scal[2]), k_lgo_wgrad and finish_objective_class (k_slabsum,
// k_epilogue).  flag_grad = 0 runs k_loo_vec mode 0, k_lgo_mask, the three LOO kernels of every chunk, k_lgo_obj and k_epilogue.
int medgp_lgo_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int32_t *group, const int32_t *ngroups,
                   int flag_grad, double *obj, double *grad, int32_t *status, int32_t *group_status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !obj || nbatch < 1) return fail(c, MEDGP_ERR_ARG, "bad argument");
    if (flag_grad & ~1) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    if (flag_grad && !grad) return fail(c, MEDGP_ERR_ARG, "grad is NULL with flag_grad set");
    int rc;
    if ((rc = check_q16(c, "medgp_lgo_grad", kWhyKinv))) return rc;
    if (!group) {   // classic LOO: medgp_loo_grad's bits
        if (ngroups) return fail(c, MEDGP_ERR_ARG, "ngroups without group ids");
        std::vector<int32_t> st((size_t)nbatch, 0);
        if ((rc = medgp_loo_grad(c, nbatch, slots, theta, flag_grad, obj, grad, st.data()))) return rc;
        int64_t at = 0;
        for (int b = 0; b < nbatch; b++) {
            if (status) status[b] = st[b];
            const int n = c->h_n[slots[b]];
            if (group_status) for (int i = 0; i < n; i++) group_status[at + i] = st[b] < 0 ? -1 : 0;
            at += n;
        }
        return MEDGP_OK;
    }
    if (!ngroups) return fail(c, MEDGP_ERR_ARG, "ngroups is NULL with group ids");
    if ((rc = check_call(c, nbatch, slots))) return rc;
    std::vector<int64_t> ooff(nbatch + 1, 0), goff(nbatch + 1, 0);   // first observation / first group of patient b in the call
    for (int b = 0; b < nbatch; b++) {
        if (ngroups[b] < 0) return fail(c, MEDGP_ERR_ARG, "ngroups[%d] = %d", b, ngroups[b]);
        ooff[b + 1] = ooff[b] + c->h_n[slots[b]];
        goff[b + 1] = goff[b] + ngroups[b];
    }
    const int64_t NO = ooff[nbatch], NG = goff[nbatch];
    if (NO > (int64_t)INT32_MAX || NG > (int64_t)INT32_MAX) return fail(c, MEDGP_ERR_ARG, "%lld observations in %lld groups in one call", (long long)NO, (long long)NG);
    for (int b = 0; b < nbatch; b++)
        for (int64_t i = ooff[b]; i < ooff[b + 1]; i++)
            if (group[i] < -1 || group[i] >= ngroups[b])
                return fail(c, MEDGP_ERR_ARG, "group[%lld] = %d outside [-1, %d) (patient %d)", (long long)i, group[i], ngroups[b], b);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    std::vector<const int *> perm(nbatch);   // internal row -> caller observation (null: the patient was uploaded grouped)
    for (int b = 0; b < nbatch; b++) perm[b] = c->h_perm_identity[slots[b]] ? nullptr : c->h_perm[slots[b]].data();
    const std::vector<TableClass> tcls = table_classes(P);
    LooTables T;
    LgoTables G;
    TableError e;
    if (!build_loo_tables(tcls, P.order.data(), P.en.data(), ooff.data(), goff.data(), nbatch, group, perm.data(), false, true, c->posterior_budget, T, e))
        return fail(c, MEDGP_ERR_CAPACITY, "patient %d: group %d of %d observations needs %zu MB at once, the budget is %zu MB (MEDGP_POSTERIOR_BUDGET_GB)",
                    e.b, e.gid, (int)e.m, e.need >> 20, c->posterior_budget >> 20);
    build_lgo_tables(tcls, P.en.data(), T, G);
    const size_t NGz = (size_t)std::max<int64_t>(NG, 1), H = c->H;
    std::vector<double> hl(NGz, (double)NAN);   // the fill of lpd: NaN where no kernel writes (a failed block; an empty group is never read)
    if ((rc = buf_ensure(c, BUF_GVEC, 4 * P.need_vec * sizeof(double)))) return rc;
    if (flag_grad && (rc = buf_ensure(c, BUF_LGO_T, P.need_mat * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_CSTAT, NGz * sizeof(int)))) return rc;
    if ((rc = buf_ensure(c, BUF_C, T.blk_need))) return rc;
    if ((rc = upload_table(c, BUF_LPD, hl))) return rc;
    if ((rc = upload_table(c, BUF_ROWS, T.rows))) return rc;
    if ((rc = upload_table(c, BUF_PATS, T.groups))) return rc;
    if ((rc = upload_table(c, BUF_PAIRS, T.pairs))) return rc;
    if ((rc = upload_table(c, BUF_BLKS, T.jobs))) return rc;
    if ((rc = upload_table(c, BUF_LGO_COLS, G.cols))) return rc;
    if ((rc = upload_table(c, BUF_LGO_TROWS, G.trows))) return rc;
    if ((rc = upload_table(c, BUF_LGO_SGL, G.sgl))) return rc;
    if ((rc = upload_table(c, BUF_LGO_ENT, G.ent))) return rc;
    if ((rc = upload_table(c, BUF_LGO_GORD, G.gord))) return rc;
    double *gvec = buf<double>(c, BUF_GVEC), *tmat = buf<double>(c, BUF_LGO_T), *d_lpd = buf<double>(c, BUF_LPD), *d_blocks = buf<double>(c, BUF_C);
    int *d_gstat = buf<int>(c, BUF_CSTAT);
    HIPCHK(c, hipMemsetAsync(d_gstat, 0, NGz * sizeof(int), c->stream));
    const LooRow *d_rows = buf<LooRow>(c, BUF_ROWS);
    const JointPat *d_groups = buf<JointPat>(c, BUF_PATS);
    const JointTile *d_pairs = buf<JointTile>(c, BUF_PAIRS), *d_jobs = buf<JointTile>(c, BUF_BLKS);
    const JointTile *d_cols = buf<JointTile>(c, BUF_LGO_COLS), *d_trows = buf<JointTile>(c, BUF_LGO_TROWS);
    const int *d_sgl = buf<int>(c, BUF_LGO_SGL), *d_ent = buf<int>(c, BUF_LGO_ENT), *d_gord = buf<int>(c, BUF_LGO_GORD);
    if ((rc = wait_lane0_staging(c))) return rc;
    if ((rc = factor_run_templated(c, nbatch, theta))) return rc;
    const double log2pi = std::log(2.0 * c->pi);
    for (size_t ci = 0; ci < P.cls.size(); ci++) {
        const SizeClass &k = P.cls[ci];
        const MedgpDev V = class_view(c, P, k);
        double *vec = gvec + 4 * k.off_vec;
        double *Tm = flag_grad ? tmat + k.off_mat : nullptr;
        const int nb = k.count, nt64 = k.nbmax;
        const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, nb, nt64);
        { Launcher l(c, KID_LOO_VEC); hipLaunchKernelGGL(k_loo_vec, dim3(4 * nt64, nb), dim3(256), 0, c->stream, V, vec, 0, log2pi); }
        { Launcher l(c, KID_LGO_VEC); hipLaunchKernelGGL(k_lgo_mask, dim3((k.ld + 255) / 256, nb), dim3(256), 0, c->stream, V, vec, d_sgl + G.sgl_off[ci], d_lpd); }
        if (flag_grad) {
            launch_kinv(c, P, k, V);
            { Launcher l(c, KID_LGO_VEC); hipLaunchKernelGGL(k_lgo_prep, dim3(nt64, 16 * nt64, nb), dim3(256), 0, c->stream, V, vec, Tm); }
        }
        for (size_t x = 0; x < T.chunks.size(); x++) {   // chunks reuse the blocks in stream order
            const LooChunk &ch = T.chunks[x];
            const LgoChunk &gc = G.chunks[x];
            if (ch.cls != (int)ci) continue;
            { Launcher l(c, KID_LOO_GRAM); hipLaunchKernelGGL(k_loo_gram, dim3(ch.npair), dim3(256), 0, c->stream, V, d_groups, d_pairs + ch.pair0, d_rows, d_blocks); }
            { Launcher l(c, KID_POSTFACTOR); hipLaunchKernelGGL(k_postfactor, dim3(ch.ng), dim3(256), 0, c->stream, V, d_groups + ch.g0, d_blocks, d_gstat); }
            {
                Launcher l(c, KID_LOO_SOLVE);
                hipLaunchKernelGGL(k_loo_solve, dim3(ch.njob), dim3(256), 0, c->stream, V, d_groups, d_jobs + ch.job0, d_rows, d_blocks, d_gstat, log2pi,
                                   (float *)nullptr, (float *)nullptr, d_lpd);
            }
            if (!flag_grad) continue;
            { Launcher l(c, KID_LGO_INV); hipLaunchKernelGGL(k_lgo_inv, dim3(gc.ncol), dim3(256), 0, c->stream, V, d_groups, d_cols + gc.col0, d_blocks, d_gstat); }
            { Launcher l(c, KID_LGO_S); hipLaunchKernelGGL(k_lgo_s, dim3(ch.npair), dim3(256), 0, c->stream, V, d_groups, d_pairs + ch.pair0, d_rows, d_blocks, d_gstat, vec); }
            { Launcher l(c, KID_LGO_T); hipLaunchKernelGGL(k_lgo_t, dim3(gc.ntrow), dim3(256), 0, c->stream, V, d_groups, d_trows + gc.trow0, d_rows, d_blocks, d_gstat, Tm); }
        }
        if (flag_grad) { Launcher l(c, KID_LOO_VEC); hipLaunchKernelGGL(k_loo_vec, dim3(4 * nt64, nb), dim3(256), 0, c->stream, V, vec, 1, log2pi); }
        { Launcher l(c, KID_LGO_VEC); hipLaunchKernelGGL(k_lgo_obj, dim3(nb), dim3(64), 0, c->stream, V, d_ent + 2 * k.b0, d_gord, d_lpd); }
        if (flag_grad)
            launch_tiles(c, KID_LGO_WGRAD, V.Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
                hipLaunchKernelGGL((k_lgo_wgrad<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, V, vec, Tm, nb, wg.wg_tiles, wg.nbp);
            });
        finish_objective_class(c, V, nb, flag_grad);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<int32_t> st((size_t)nbatch, 0);
    std::vector<int> gst(NGz, 0);
    if ((rc = download_objective(c, nbatch, flag_grad, obj, grad, st.data(), gst.data(), d_gstat, sizeof(int) * (size_t)NG))) return rc;
    for (int b = 0; b < nbatch; b++) {
        if (status) status[b] = st[b];
        bool bad = false;
        for (int64_t g = goff[b]; g < goff[b + 1]; g++) {
            const bool gb = st[b] < 0 || gst[(size_t)g] < 0;
            if (group_status) group_status[g] = gb ? -1 : 0;
            bad = bad || gb;
        }
        if (bad && st[b] >= 0) {   // a group whose block met a bad pivot: the patient's J and gradient are not defined
            obj[b] = (double)NAN;
            if (flag_grad) for (size_t h = 0; h < H; h++) grad[(size_t)b * H + h] = (double)NAN;
        }
    }
    return MEDGP_OK;
}

// Products of the Fisher information with nvec directions per entry (kernels_fisher.h).  ONE pipeline run in the grouped order (as
// medgp_loo_grad: factor, U = L^-T), then per size class k_loo_kinv (P = U U^T into the dead Kmat block).  Then, direction by
// direction, per size class in stream order: launch_kdot (k_fisher_prep, k_fisher_kdot), k_fisher_t (T = P Kdot), k_fisher_wgrad
// (W_F tiles -> slab, wdiag), k_slabsum and k_epilogue (EPI_BARE).  Kdot and T are buffers of the call, reused by every direction;
// every direction runs the same launches with the same geometry, so its bits depend neither on nvec nor on its position.  The four
// matrices of every entry are alive at once: a call that needs more than the memory budget is refused (fisher_tables.h), there are
// no memory waves.
int medgp_fisher_vec(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int nvec, const double *vec, double *fvec,
                     int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !vec || !fvec) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (nvec < 1) return fail(c, MEDGP_ERR_ARG, "nvec = %d", nvec);
    int rc;
    if ((rc = check_q16(c, "medgp_fisher_vec", kWhyKinv))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = check_one_wave(c, fisher_fits(P.need_mat, c->rules.mem_budget), FISHER_MATS, ""))) return rc;
    const size_t H = c->H;
    const FisherBuffers fb = fisher_buffers(P.need_mat, nbatch, nvec, (int)H, c->rules.Q, c->rules.D);
    if ((rc = buf_ensure(c, BUF_FI_KDOT, fb.mat_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_T, fb.mat_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_COEF, fb.coef_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_DIR, fb.dir_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_OUT, fb.dir_doubles * sizeof(double)))) return rc;
    double *kdot = buf<double>(c, BUF_FI_KDOT), *tmat = buf<double>(c, BUF_FI_T), *coef = buf<double>(c, BUF_FI_COEF);
    double *d_dir = buf<double>(c, BUF_FI_DIR), *d_out = buf<double>(c, BUF_FI_OUT);
    if ((rc = wait_lane0_staging(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_dir, vec, fb.dir_doubles * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = factor_run_templated(c, nbatch, theta))) return rc;
    for (const SizeClass &k : P.cls) launch_kinv(c, P, k, class_view(c, P, k));
    for (int j = 0; j < nvec; j++)
        for (const SizeClass &k : P.cls) {
            const MedgpDev V = class_view(c, P, k);
            const int nb = k.count;
            double *Kd = kdot + k.off_mat, *Tm = tmat + k.off_mat, *cf = coef + (size_t)k.b0 * V.hyp_stride;
            const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, nb, k.nbmax);
            launch_kdot(c, V, k, d_dir, nvec, j, cf, Kd);
            launch_fisher_t(c, V, k, Kd, Tm);
            launch_tiles(c, KID_FI_WGRAD, V.Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
                hipLaunchKernelGGL((k_fisher_wgrad<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, V, Tm, nb, wg.wg_tiles, wg.nbp);
            });
            launch_slabsum(c, c->stream, V, nb);
            launch_epilogue(c, c->stream, V, nb, c->d_theta, 1, 1, c->d_nlml, d_out + (size_t)j * nbatch * H, c->d_status_out, EPI_BARE);
        }
    HIPCHK(c, hipGetLastError());
    std::vector<double> out;
    if ((rc = download_directions(c, d_out, fb.dir_doubles, out))) return rc;
    if ((rc = download_objective(c, nbatch, 0, nullptr, nullptr, status))) return rc;
    transpose_directions(out, nbatch, nvec, H, fvec);
    return MEDGP_OK;
}

// Products of the exact Hessian of the data term of the nlml with nvec directions per entry (kernels_hess.h).  ONE pipeline run as
// medgp_fisher_vec (factor, U = L^-T, alpha), then per size class k_loo_kinv (P into the dead Kmat block) and the W pass: k_hess_moments
// (S, SM, SV pieces -> the gradient slab, diag(W), M3 / M4 pieces -> the call's two-plane slab), k_slabsum on a view whose block sums
// and wdiag are buffers of the call, k_hess_slabsum; with `grad`, k_epilogue's gradient lines on that view (no prior, no scalar).
// Then, direction by direction, per size class in stream order: k_fisher_prep, k_fisher_kdot, k_fisher_t, k_hess_beta (beta = T alpha),
// k_hess_wgrad (Wdot tiles -> slab, wdiag), k_slabsum and k_hess_epilogue.  Every direction runs the same launches with the same
// geometry, so its bits depend neither on nvec nor on its position.  Capacity as the Fisher call (hess_tables.h): no memory waves.
int medgp_hess_vec(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int nvec, const double *vec, double *hvec,
                   double *grad, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !vec || !hvec) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (nvec < 1) return fail(c, MEDGP_ERR_ARG, "nvec = %d", nvec);
    int rc;
    if ((rc = check_q16(c, "medgp_hess_vec", kWhyKinv))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = check_one_wave(c, hess_fits(P.need_mat, c->rules.mem_budget), HESS_MATS, ""))) return rc;
    const size_t H = c->H, QDD = (size_t)c->rules.Q * c->rules.D * c->rules.D;
    const HessBuffers hb = hess_buffers(P.need_mat, P.need_vec, P.need_slab, nbatch, nvec, (int)H, c->rules.Q, c->rules.D);
    if ((rc = buf_ensure(c, BUF_FI_KDOT, hb.mat_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_T, hb.mat_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_COEF, hb.coef_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_DIR, hb.dir_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_OUT, hb.dir_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_HE_SLAB, hb.hislab_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_HE_SUMS, hb.sums_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_HE_VEC, hb.vec_doubles * sizeof(double)))) return rc;
    double *kdot = buf<double>(c, BUF_FI_KDOT), *tmat = buf<double>(c, BUF_FI_T), *coef = buf<double>(c, BUF_FI_COEF);
    double *d_dir = buf<double>(c, BUF_FI_DIR), *d_out = buf<double>(c, BUF_FI_OUT);
    double *hislab = buf<double>(c, BUF_HE_SLAB), *sums = buf<double>(c, BUF_HE_SUMS), *hvecs = buf<double>(c, BUF_HE_VEC);
    if ((rc = wait_lane0_staging(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_dir, vec, hb.dir_doubles * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = factor_run_templated(c, nbatch, theta))) return rc;
    // the view of the W pass of a class: block sums and diag(W) in the call's own buffers, the direction's view keeps the context's
    auto w_view = [&](const MedgpDev &V, const SizeClass &k) {
        MedgpDev W = V;
        W.S = sums + (size_t)k.b0 * QDD; W.SM = W.S + (size_t)nbatch * QDD; W.SV = W.SM + (size_t)nbatch * QDD;
        W.wdiag = hvecs + P.need_vec + k.off_vec;
        return W;
    };
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k), W = w_view(V, k);
        const int nb = k.count;
        const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, nb, k.nbmax);
        double *hi = hislab + hess_hislab_of(k.off_slab), *M3 = sums + (3 * (size_t)nbatch + k.b0) * QDD, *M4 = M3 + (size_t)nbatch * QDD;
        launch_kinv(c, P, k, V);
        launch_tiles(c, KID_HE_MOMENTS, V.Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
            hipLaunchKernelGGL((k_hess_moments<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, W, hi, nb, wg.wg_tiles, wg.nbp);
        });
        launch_slabsum(c, c->stream, W, nb);
        { Launcher l(c, KID_HE_SLABSUM); hipLaunchKernelGGL(k_hess_slabsum, dim3(nb, hess_slabsum_grid(V.Q, V.D)), dim3(256), 0, c->stream, W, hi, M3, M4); }
        if (grad) launch_epilogue(c, c->stream, W, nb, c->d_theta, 1, 1, c->d_nlml, c->d_grad, c->d_status_out, EPI_BARE);
    }
    for (int j = 0; j < nvec; j++)
        for (const SizeClass &k : P.cls) {
            const MedgpDev V = class_view(c, P, k), W = w_view(V, k);
            const int nb = k.count, nt64 = k.nbmax;
            double *Kd = kdot + k.off_mat, *Tm = tmat + k.off_mat, *cf = coef + (size_t)k.b0 * V.hyp_stride, *beta = hvecs + k.off_vec;
            const HessW hw{W.S, W.SM, W.SV, W.SV + (size_t)nbatch * QDD, W.SV + 2 * (size_t)nbatch * QDD, W.wdiag};
            const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, nb, nt64);
            launch_kdot(c, V, k, d_dir, nvec, j, cf, Kd);
            launch_fisher_t(c, V, k, Kd, Tm);
            { Launcher l(c, KID_HE_BETA); hipLaunchKernelGGL(k_hess_beta, dim3(hess_beta_grid(nt64), nb), dim3(256), 0, c->stream, V, Tm, beta); }
            launch_tiles(c, KID_HE_WGRAD, V.Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
                hipLaunchKernelGGL((k_hess_wgrad<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, V, Tm, beta, nb, wg.wg_tiles, wg.nbp);
            });
            launch_slabsum(c, c->stream, V, nb);
            const dim3 eg(nb, epilogue_parts(nb, c->rules.num_cu, V.H, MEDGP_EPI_PARTS));
            Launcher l(c, KID_HE_EPILOGUE);
            hipLaunchKernelGGL(k_hess_epilogue, eg, dim3(256), 0, c->stream, V, hw, c->d_theta, d_dir, nvec, j, cf,
                               d_out + (size_t)j * nbatch * H, c->d_status_out);
        }
    HIPCHK(c, hipGetLastError());
    std::vector<double> out;
    if ((rc = download_directions(c, d_out, hb.dir_doubles, out))) return rc;
    if ((rc = download_objective(c, nbatch, 1, nullptr, grad, status))) return rc;
    transpose_directions(out, nbatch, nvec, H, hvec);
    return MEDGP_OK;
}

// Directional derivatives of the posterior in the hypers (kernels_posterior_jvp.h).  ONE pipeline run in the grouped order (factor,
// U = L^-T, alpha), then per size class and launch chunk of its tiles, in stream order: k_pjvp_solve (W = P K* into the chunk's work
// rows, mean, var) and, direction by direction, k_fisher_prep, k_fisher_kdot, k_pjvp_u (u = Kdot alpha) and k_pjvp_dir.  A class has one
// chunk unless its work rows exceed MEDGP_POSTERIOR_BUDGET_GB; then every chunk forms the direction's Kdot again (the same bits).  Kdot,
// the coefficient blocks and u are buffers of the call, reused by every direction; every direction runs the same launches with the
// same geometry.  L is never overwritten.  The three matrices of every entry are alive at once: a call that needs more than the memory
// budget is refused (pjvp_tables.h), there are no memory waves.
int medgp_posterior_jvp_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                              const int32_t *meta2, const float *t2, int nvec, const double *vec, float *mean, float *var, double *dmean,
                              double *dvar, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !offsets || !vec || !dmean || !dvar) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (nvec < 1) return fail(c, MEDGP_ERR_ARG, "nvec = %d", nvec);
    if ((mean == nullptr) != (var == nullptr)) return fail(c, MEDGP_ERR_ARG, "mean and var: both or neither");
    int rc;
    if ((rc = check_q16(c, "medgp_posterior_jvp_batch", nullptr))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    // (mean / var are optional here: the per-point outputs the call requires are dmean / dvar, checked above)
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, false, "dmean / dvar");
    if (M < 0) return (int)M;
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, nullptr, ht2, hm2);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = check_one_wave(c, pjvp_fits(P.need_mat, c->rules.mem_budget), PJVP_MATS, ""))) return rc;
    const size_t H = c->H;
    const PjvpBuffers pb = pjvp_buffers(P.need_mat, P.need_vec, nbatch, nvec, (int)H, c->rules.Q, c->rules.D, M);
    PointTables<PostTile> T;
    build_pjvp_tiles(table_classes(P), P.order.data(), offsets, c->posterior_budget, T);
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_KDOT, pb.mat_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_COEF, pb.coef_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_FI_DIR, pb.dir_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_PJ_U, std::max<size_t>(pb.u_doubles, 1) * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_PJ_OUT, pb.out_doubles * sizeof(double)))) return rc;
    double *kdot = buf<double>(c, BUF_FI_KDOT), *coef = buf<double>(c, BUF_FI_COEF), *d_dir = buf<double>(c, BUF_FI_DIR);
    double *uvec = buf<double>(c, BUF_PJ_U), *d_dmean = buf<double>(c, BUF_PJ_OUT), *d_dvar = d_dmean + pjvp_dvar_offset(M, nvec);
    HIPCHK(c, hipMemcpyAsync(d_dir, vec, pb.dir_doubles * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = factor_run_templated(c, nbatch, theta))) return rc;   // (its results travel through buffers of its own: no wait for lane 0's staging)
    for (const TileChunk &ch : T.chunks) {   // chunks reuse the work rows in stream order
        const SizeClass &k = P.cls[ch.cls];
        const MedgpDev V = class_view(c, P, k);
        const int nb = k.count, nt64 = k.nbmax;
        const PostTile *tiles = buf<PostTile>(c, BUF_TILES) + ch.t0;
        double *Kd = kdot + k.off_mat, *cf = coef + (size_t)k.b0 * V.hyp_stride, *u = uvec + k.off_vec;
        launch_pjvp_solve(c, V, tiles, ch.nt, ch.stride, nvec, d_dmean, d_dvar);
        for (int j = 0; j < nvec; j++) {
            launch_kdot(c, V, k, d_dir, nvec, j, cf, Kd);
            { Launcher l(c, KID_PJ_U); hipLaunchKernelGGL(k_pjvp_u, dim3(pjvp_u_grid(nt64), nb), dim3(256), 0, c->stream, V, Kd, u); }
            Launcher l(c, KID_PJ_DIR);
            hipLaunchKernelGGL(k_pjvp_dir, dim3(ch.nt), dim3(256), 0, c->stream, V, tiles, buf<int>(c, BUF_META2), buf<double>(c, BUF_T2), buf<double>(c, BUF_WORK),
                               ch.stride, cf, Kd, u, nvec, j, d_dmean, d_dvar);
        }
    }
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair<double>(c, M * nvec, d_dmean, d_dvar, dmean, dvar))) return rc;
    if ((rc = download_pair(c, M, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), mean, var))) return rc;
    return read_status(c, nbatch, status);
}

// The gradient of a loss of the predictions in the hypers (kernels_posterior_vjp.h).  ONE pipeline run in the grouped order (factor,
// U = L^-T, z, alpha), then per size class and launch chunk of whole entries, in stream order: k_pjvp_solve (W = P K* and V = L^-1 K*
// into the chunk's work rows, mean, var) and, cotangent set by set, k_pvjp_cot, k_pvjp_wgrad (G tiles -> slab, wdiag), the nlml
// gradient's own k_slabsum, k_pvjp_cross (rectangular sums and the test diagonal folded into S, SM, SV), k_epilogue told to leave the
// prior and the scalar out, and k_pvjp_finish.  Every set runs the same launches with the same geometry.  The points travel sorted by
// covariate inside every patient (pvjp_tables.h); mean and var go back in the caller's order.  L, U and alpha are never overwritten.
int medgp_posterior_vjp_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                              const int32_t *meta2, const float *t2, int loss_kind, const double *y2, const double *wt, int ncot,
                              const double *cot_mean, const double *cot_var, float *mean, float *var, double *loss, double *grad,
                              int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !offsets || !grad) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    c->pv_valid = false;
    if (loss_kind < MEDGP_PLOSS_CUSTOM || loss_kind > MEDGP_PLOSS_CRPS) return fail(c, MEDGP_ERR_ARG, "unknown loss_kind %d", loss_kind);
    if (ncot < 1) return fail(c, MEDGP_ERR_ARG, "ncot = %d", ncot);
    if ((mean == nullptr) != (var == nullptr)) return fail(c, MEDGP_ERR_ARG, "mean and var: both or neither");
    const bool builtin = loss_kind != MEDGP_PLOSS_CUSTOM;
    if (builtin && ncot != 1) return fail(c, MEDGP_ERR_ARG, "ncot = %d with a built-in loss (1 expected)", ncot);
    if (builtin && (cot_mean || cot_var)) return fail(c, MEDGP_ERR_ARG, "cot_mean / cot_var given with a built-in loss");
    if (builtin && (!loss || !y2)) return fail(c, MEDGP_ERR_ARG, "loss / y2 is NULL with a built-in loss");
    if (!builtin && (!cot_mean || !cot_var)) return fail(c, MEDGP_ERR_ARG, "cot_mean / cot_var is NULL with MEDGP_PLOSS_CUSTOM");
    if (!builtin && (loss || y2 || wt)) return fail(c, MEDGP_ERR_ARG, "loss / y2 / wt given with MEDGP_PLOSS_CUSTOM");
    int rc;
    if ((rc = check_q16(c, "medgp_posterior_vjp_batch", nullptr))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    // (mean / var are optional here; the per-point inputs the call requires, named for the message, were checked above; the covariates
    //  are range-checked here, before the tables sort by them)
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, false, builtin ? "y2" : "cot_mean / cot_var");
    if (M < 0) return (int)M;
    const int D = c->rules.D, Q = c->rules.Q;
    const bool lmc = c->kidx == MEDGP_KERNEL_LMC_SM;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = check_one_wave(c, pvjp_fits(P.need_mat, c->rules.mem_budget), PVJP_MATS, ""))) return rc;
    PvjpTables T;
    TableError terr{};
    if (!build_pvjp_tables(table_classes(P), P.order.data(), offsets, (lmc && M > 0) ? meta2 : nullptr, nbatch, D, c->posterior_budget, T, terr))
        return fail(c, MEDGP_ERR_CAPACITY, "patient %d: the work rows of its %lld test points (%zu MB) exceed the budget of %zu MB (MEDGP_POSTERIOR_BUDGET_GB): split its points",
                    terr.b, terr.m, terr.need >> 20, c->posterior_budget >> 20);
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, T.src.data(), ht2, hm2);
    const size_t H = c->H, Mz = pvjp_mz(M);
    const PvjpBuffers pb = pvjp_buffers(P.need_vec, nbatch, ncot, (int)H, Q, D, M);
    // the caller's per-point inputs in the device's point order, the cotangent sets set-major
    std::vector<double> hin(pb.in_doubles, 0.0);
    for (int64_t k = 0; k < M; k++) {
        const int64_t j = T.src[(size_t)k];
        if (builtin) {
            hin[2 * Mz + (size_t)k] = y2[j];
            hin[3 * Mz + (size_t)k] = wt ? wt[j] : 1.0;
        } else
            for (int s = 0; s < ncot; s++) {
                hin[(size_t)s * Mz + (size_t)k] = cot_mean[(size_t)j * ncot + s];
                hin[((size_t)ncot + s) * Mz + (size_t)k] = cot_var[(size_t)j * ncot + s];
            }
    }
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = upload_table(c, BUF_PV_ENT, T.ents))) return rc;
    if ((rc = upload_table(c, BUF_PV_SEG, T.pseg))) return rc;
    if ((rc = upload_table(c, BUF_PV_ORD, T.dev_of))) return rc;
    if ((rc = upload_table(c, BUF_PV_IN, hin))) return rc;
    if ((rc = buf_ensure(c, BUF_PV_ORD, sizeof(int)))) return rc;   // (a call without points: the kernels still take the pointer)
    if ((rc = buf_ensure(c, BUF_PV_PTS, pb.pts_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_PV_VEC, pb.vec_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_PV_SMALL, pb.small_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_PV_OUT, pb.out_doubles * sizeof(double)))) return rc;
    const PvjpEnt *d_ents = buf<PvjpEnt>(c, BUF_PV_ENT);
    const int *d_pseg = buf<int>(c, BUF_PV_SEG), *d_ord = buf<int>(c, BUF_PV_ORD), *d_meta2 = buf<int>(c, BUF_META2);
    const double *d_in = buf<double>(c, BUF_PV_IN), *d_t2 = buf<double>(c, BUF_T2);
    double *d_pts = buf<double>(c, BUF_PV_PTS), *d_cvec = buf<double>(c, BUF_PV_VEC), *d_small = buf<double>(c, BUF_PV_SMALL);
    double *d_out = buf<double>(c, BUF_PV_OUT), *d_work = buf<double>(c, BUF_WORK);
    if ((rc = wait_lane0_staging(c))) return rc;
    if ((rc = factor_run_templated(c, nbatch, theta))) return rc;
    for (const PvjpChunk &ch : T.chunks) {   // chunks reuse the work rows in stream order
        const SizeClass &k = P.cls[ch.cls];
        const MedgpDev V = class_view(c, P, k), Vc = shifted_view(V, ch.e0);
        const int nb = ch.ne, nt64 = k.nbmax;
        // a view without bpos takes the entry index as the caller's row: the rows of the shifted view then start ch.e0 further
        const size_t row0 = Vc.bpos ? 0 : (size_t)ch.e0;
        const PvjpEnt *ents = d_ents + k.b0 + ch.e0;
        double *small = d_small + (size_t)(k.b0 + ch.e0) * (D + 2), *cvec = d_cvec + k.off_vec + (size_t)ch.e0 * k.ld;
        if (ch.nt > 0) launch_pjvp_solve(c, V, buf<PostTile>(c, BUF_TILES) + ch.t0, ch.nt, ch.stride, 0, nullptr, nullptr);
        const WgradGrid wg = wgrad_grid(P.en.data() + k.b0 + ch.e0, nb, nt64);
        for (int s = 0; s < ncot; s++) {
            double *g = d_out + ((size_t)s * nbatch + row0) * H;
            {
                Launcher l(c, KID_PV_COT);
                hipLaunchKernelGGL(k_pvjp_cot, dim3(nb), dim3(256), 0, c->stream, Vc, ents, d_meta2, d_t2, d_ord, d_work, ch.stride, d_in, d_pts, cvec, small,
                                   Mz, loss_kind, ncot, s, wt ? 1 : 0);
            }
            launch_tiles(c, KID_PV_WGRAD, Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
                hipLaunchKernelGGL((k_pvjp_wgrad<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, Vc, ents, d_work, ch.stride,
                                   d_pts + Mz, cvec, nb, wg.wg_tiles, wg.nbp);
            });
            launch_slabsum(c, c->stream, Vc, nb);
            {
                Launcher l(c, KID_PV_CROSS);
                hipLaunchKernelGGL(k_pvjp_cross, dim3(pvjp_cross_grid(D), nb), dim3(256), 0, c->stream, Vc, ents, d_pseg, d_t2, d_work, ch.stride, d_pts, small, Mz);
            }
            launch_epilogue(c, c->stream, Vc, nb, c->d_theta + row0 * H, 1, 1, c->d_nlml, g, c->d_status_out + row0, EPI_BARE);
            Launcher l(c, KID_PV_FINISH);
            hipLaunchKernelGGL(k_pvjp_finish, dim3(nb), dim3(256), 0, c->stream, Vc, small, g, builtin ? 1 : 0);
        }
    }
    HIPCHK(c, hipGetLastError());
    std::vector<double> out, hsmall(pb.small_doubles);
    std::vector<float> hmv;
    std::vector<int32_t> st(nbatch);
    if ((rc = download_directions(c, d_out, pb.out_doubles, out))) return rc;
    if (builtin) HIPCHK(c, hipMemcpyAsync(hsmall.data(), d_small, pb.small_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if ((rc = download_pair(c, M, buf<float>(c, BUF_MEAN), buf<float>(c, BUF_VAR), mean, var, &hmv))) return rc;
    if ((rc = read_status(c, nbatch, st.data()))) return rc;
    free_retired(c);
    transpose_directions(out, nbatch, ncot, H, grad);
    // (the loss of a failed entry is the NaN k_pvjp_cot left in its block: the scatter's NaN has the same bits)
    if (builtin) scatter_entry_blocks(P.order.data(), st.data(), nbatch, hsmall.data(), (size_t)D + 2, {{(size_t)D, 1, loss}});
    unsort_pair(hmv, T.src.data(), mean, var);
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * nbatch);
    c->pv_src = std::move(T.src);
    c->pv_valid = true;
    return MEDGP_OK;
}

// the fp64 mean and var the last medgp_posterior_vjp_batch formed its cotangents from, in the caller's point order
int medgp_posterior_vjp_moments(medgp_ctx *c, int64_t M, double *mean, double *var) {
    if (!c) return MEDGP_ERR_ARG;
    if (!c->pv_valid) return fail(c, MEDGP_ERR_ARG, "no medgp_posterior_vjp_batch before this call");
    if (M != (int64_t)c->pv_src.size()) return fail(c, MEDGP_ERR_ARG, "M = %lld, the last call had %zu points", (long long)M, c->pv_src.size());
    if (M == 0) return MEDGP_OK;
    if (!mean || !var) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<double> h(2 * (size_t)M);
    const double *d = buf<double>(c, BUF_PV_PTS) + pvjp_moments_offset(c->rules.Q, M);
    HIPCHK(c, hipMemcpyAsync(h.data(), d, 2 * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsort_pair(h, c->pv_src.data(), mean, var);
    return MEDGP_OK;
}

}  // extern "C"

namespace {

// What the two baseline calls share (kernels_mean.h): the argument checks, the plan, the capacity rule, the call's buffers, [b0 | lam] to
// the device, ONE pipeline run in the grouped order (factor, U = L^-T, z, alpha; min_n as the caller's family has it) and, per size
// class in stream order, k_mean_g (G = L^-1 H) and k_mean_small (A, its factor, beta^, A^-1, dmean, the objective -> scal[2]; status -1
// for an improper entry or a failed pivot of A).
// The two basis calls (kernels_basis.h) share all of it with H from the resident store: basis = true takes the column count p from the
// slots' bases (all the same, else MEDGP_ERR_ARG, as for a slot without a basis: before any device work), sends every entry's offset
// into the store beside [b0 | lam], and launches k_basis_g / k_basis_small in the two kernels' places.  mc.ncol: D or p.
struct MeanCall {
    MeanBuffers mb;
    double *G, *PH, *Pm, *vec, *small, *in;
    int ncol;
};
int mean_prepare(medgp_ctx *c, const char *who, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0,
                 const double *lam, int min_n, bool basis, MeanCall &mc) {
    if (!slots || !theta || !b0) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (mode != MEDGP_MEAN_MARGINAL && mode != MEDGP_MEAN_FIXED) return fail(c, MEDGP_ERR_ARG, "unknown mode %d", mode);
    if (mode == MEDGP_MEAN_MARGINAL && !lam) return fail(c, MEDGP_ERR_ARG, "lam is NULL with MEDGP_MEAN_MARGINAL");
    int rc;
    if ((rc = check_q16(c, who, nullptr))) return rc;
    if (!basis && c->rules.D > MEAN_MAX_D) return fail(c, MEDGP_ERR_CAPACITY, "%s supports D <= %d covariates (D = %d): the rank-D correction is one 64-column panel", who, MEAN_MAX_D, c->rules.D);
    if ((rc = check_call(c, nbatch, slots))) return rc;
    int D = c->rules.D;   // the column count of H
    if (basis) {
        for (int b = 0; b < nbatch; b++) {
            if (!c->basis.has(slots[b])) return fail(c, MEDGP_ERR_ARG, "slots[%d] = %d has no basis (medgp_set_basis; a new patient drops it)", b, slots[b]);
            if (c->basis.slot[slots[b]].p != c->basis.slot[slots[0]].p)
                return fail(c, MEDGP_ERR_ARG, "slots[%d] = %d carries a basis of %d columns, slots[0] one of %d: one p per call", b, slots[b], c->basis.slot[slots[b]].p, c->basis.slot[slots[0]].p);
        }
        D = c->basis.slot[slots[0]].p;
    }
    mc.ncol = D;
    for (size_t i = 0; i < (size_t)nbatch * D; i++) {
        if (!std::isfinite(b0[i])) return fail(c, MEDGP_ERR_ARG, "b0[%zu] = %g is not finite", i, b0[i]);
        if (mode == MEDGP_MEAN_MARGINAL && !(lam[i] >= 0.0 && std::isfinite(lam[i]))) return fail(c, MEDGP_ERR_ARG, "lam[%zu] = %g: a precision is finite and >= 0", i, lam[i]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = check_one_wave(c, mean_fits(P.need_mat, P.need_vec, c->rules.mem_budget), MEAN_MATS, " and panels"))) return rc;
    mc.mb = mean_buffers(P.need_vec, nbatch, D);
    if ((rc = buf_ensure(c, BUF_MN_G, mc.mb.panel_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_MN_PH, mc.mb.panel_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_MN_PM, mc.mb.panel_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_MN_VEC, mc.mb.vec_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_MN_SMALL, mc.mb.small_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_MN_IN, mc.mb.in_doubles * sizeof(double)))) return rc;
    mc.G = buf<double>(c, BUF_MN_G); mc.PH = buf<double>(c, BUF_MN_PH); mc.Pm = buf<double>(c, BUF_MN_PM);
    mc.vec = buf<double>(c, BUF_MN_VEC); mc.small = buf<double>(c, BUF_MN_SMALL); mc.in = buf<double>(c, BUF_MN_IN);
    if ((rc = wait_lane0_staging(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(mc.in, b0, sizeof(double) * nbatch * D, hipMemcpyHostToDevice, c->stream));
    if (mode == MEDGP_MEAN_MARGINAL)
        HIPCHK(c, hipMemcpyAsync(mc.in + mean_lam_offset(nbatch, D), lam, sizeof(double) * nbatch * D, hipMemcpyHostToDevice, c->stream));
    if (basis) {   // (through the pinned ring: the table is the call's own)
        if ((rc = buf_ensure(c, BUF_BS_OFF, sizeof(long long) * nbatch))) return rc;
        void *pin = nullptr;
        if ((rc = pin_stage(c, sizeof(long long) * nbatch, &pin))) return rc;
        for (int b = 0; b < nbatch; b++) ((long long *)pin)[b] = c->basis.slot[slots[b]].off;
        HIPCHK(c, hipMemcpyAsync(buf<long long>(c, BUF_BS_OFF), pin, sizeof(long long) * nbatch, hipMemcpyHostToDevice, c->stream));
    }
    if ((rc = factor_run_templated(c, nbatch, theta, min_n))) return rc;
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        double *Gk = mc.G + MEAN_PW * k.off_vec;
        double *wk = mc.vec + k.off_vec, *sk = mc.small + (size_t)k.b0 * mean_small_stride(D);
        if (basis) {
            Launcher l(c, KID_BS_G);
            const dim3 grid(basis_g_grid(k.nbmax), k.count);
            const long long *hoff = buf<long long>(c, BUF_BS_OFF);
            switch ((D + 15) / 16) {   // the column tiles of the panel that carry columns
            case 1: hipLaunchKernelGGL(k_basis_g<1>, grid, dim3(256), 0, c->stream, V, c->d_basis, hoff, D, Gk); break;
            case 2: hipLaunchKernelGGL(k_basis_g<2>, grid, dim3(256), 0, c->stream, V, c->d_basis, hoff, D, Gk); break;
            case 3: hipLaunchKernelGGL(k_basis_g<3>, grid, dim3(256), 0, c->stream, V, c->d_basis, hoff, D, Gk); break;
            default: hipLaunchKernelGGL(k_basis_g<4>, grid, dim3(256), 0, c->stream, V, c->d_basis, hoff, D, Gk); break;
            }
        } else {
            Launcher l(c, KID_MN_G);
            hipLaunchKernelGGL(k_mean_g, dim3(mean_g_grid(k.nbmax), k.count), dim3(256), 0, c->stream, V, Gk);
        }
        Launcher l(c, basis ? KID_BS_SMALL : KID_MN_SMALL);   // (one body, fe_small_body, behind both)
        if (basis) hipLaunchKernelGGL(k_basis_small, dim3(k.count), dim3(256), 0, c->stream, V, Gk, mc.in, nbatch, mode, D, wk, sk);
        else hipLaunchKernelGGL(k_mean_small, dim3(k.count), dim3(256), 0, c->stream, V, Gk, mc.in, nbatch, mode, wk, sk);
    }
    return MEDGP_OK;
}

// beta, dmean and beta_cov of the call from the downloaded per-entry blocks (internal order) to the caller's rows; NaN for failed entries
void mean_scatter(const BatchPlan &P, const std::vector<double> &hs, const int32_t *st, int nbatch, int D, double *dmean, double *beta, double *beta_cov) {
    const size_t n = (size_t)D;
    scatter_entry_blocks(P.order.data(), st, nbatch, hs.data(), mean_small_stride(D),
                         {{mean_off_beta(D), n, beta}, {mean_off_dmean(D), n, dmean}, {mean_off_cov(D), n * n, beta_cov}});
}

// The nlml with a constant baseline per covariate, fixed or integrated out, and its gradients (kernels_mean.h).  mean_prepare, then per
// size class in stream order, for a gradient: k_mean_panel (PH = U G on fp64 MFMA, Pm, alpha~), k_mean_wgrad (W~ tiles -> slab, wdiag) on
// a view whose alpha is alpha~; then finish_objective_class (k_slabsum, k_epilogue: the objective k_mean_small left in scal[2], to which
// it adds the priors on theta).  flag_grad = 0 runs mean_prepare and k_epilogue only.  L, U, z and alpha are never overwritten.
// basis: medgp_basis_nlml_grad -- the same launches on p columns (k_mean_panel reads its column count from the view's D: it is handed
// a view whose D is p; the gradient pass and the epilogue keep the covariate count).
int mean_grad_impl(medgp_ctx *c, const char *who, bool basis, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0,
                   const double *lam, int flag_grad, double *nlml, double *grad, double *dmean, double *beta, double *beta_cov, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (flag_grad & ~1) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    MeanCall mc{};
    int rc;
    if ((rc = mean_prepare(c, who, nbatch, slots, theta, mode, b0, lam, 3, basis, mc))) return rc;
    const BatchPlan &P = c->plan;
    const int D = mc.ncol;   // the columns of H
    for (const SizeClass &k : P.cls) {
        MedgpDev V = class_view(c, P, k);
        const int nb = k.count, nt64 = k.nbmax;
        if (flag_grad) {
            double *Gk = mc.G + MEAN_PW * k.off_vec, *PHk = mc.PH + MEAN_PW * k.off_vec, *Pmk = mc.Pm + MEAN_PW * k.off_vec;
            double *at = mc.vec + mean_alpha_offset(P.need_vec) + k.off_vec;
            {
                Launcher l(c, KID_MN_PANEL);
                MedgpDev Vp = V;
                Vp.D = D;
                hipLaunchKernelGGL(k_mean_panel, dim3(mean_panel_grid(nt64), nb), dim3(256), 0, c->stream, Vp, Gk, mc.small + (size_t)k.b0 * mean_small_stride(D), mode, PHk, Pmk, at);
            }
            V.alpha = at;   // the gradient pass and what follows see alpha~
            const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, nb, nt64);
            const int k1 = mode == MEDGP_MEAN_MARGINAL ? mean_wgrad_k1(D, WG_KC) : 0;
            launch_tiles(c, KID_MN_WGRAD, V.Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
                hipLaunchKernelGGL((k_mean_wgrad<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, V, Pmk, k1, nb, wg.wg_tiles, wg.nbp);
            });
        }
        finish_objective_class(c, V, nb, flag_grad);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<double> hs(mc.mb.small_doubles);
    std::vector<int32_t> st(nbatch);
    if ((rc = download_objective(c, nbatch, flag_grad, nlml, grad, st.data(), hs.data(), mc.small, mc.mb.small_doubles * sizeof(double)))) return rc;
    mean_scatter(P, hs, st.data(), nbatch, D, dmean, beta, beta_cov);
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * nbatch);
    return MEDGP_OK;
}

// The posterior at test points under the same model (kernels_mean.h).  mean_prepare (no n > 2 guard, as medgp_posterior_batch), then per
// launch chunk of tiles of 64 points, in stream order: the unchanged k_pjvp_solve (V = L^-1 K* behind the first panel of every tile's
// work rows) and k_mean_post (G^T V on fp64 MFMA, mean, var in fp64).  The points keep the caller's order.
// basis: medgp_basis_posterior_batch -- k_basis_post in k_mean_post's place, with the points' basis rows h2 ([M][p], finite).
int mean_post_impl(medgp_ctx *c, const char *who, bool basis, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0,
                   const double *lam, const int64_t *offsets, const int32_t *meta2, const float *t2, const double *h2, double *mean, double *var,
                   double *beta, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!offsets) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (nbatch < 1) return fail(c, MEDGP_ERR_CAPACITY, "nbatch %d", nbatch);
    int rc;
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, false, nullptr);   // (mean / var are optional)
    if (M < 0) return (int)M;
    if ((mean == nullptr) != (var == nullptr)) return fail(c, MEDGP_ERR_ARG, "mean and var: both or neither");
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, nullptr, ht2, hm2);
    MeanCall mc{};
    if (basis && M > 0) {   // (p from the first slot's basis; mean_prepare refuses what is wrong with the slots)
        if (!h2) return fail(c, MEDGP_ERR_ARG, "h2 is NULL");
        if (!slots) return fail(c, MEDGP_ERR_ARG, "NULL argument");
        if ((rc = check_call(c, nbatch, slots))) return rc;
        const size_t p = c->basis.has(slots[0]) ? c->basis.slot[slots[0]].p : 0;
        for (size_t i = 0; i < (size_t)M * p; i++)
            if (!std::isfinite(h2[i])) return fail(c, MEDGP_ERR_ARG, "h2[%zu] = %g is not finite", i, h2[i]);
    }
    if ((rc = mean_prepare(c, who, nbatch, slots, theta, mode, b0, lam, 1, basis, mc))) return rc;
    const BatchPlan &P = c->plan;
    const int D = mc.ncol;   // the columns of H
    if (basis && M > 0) {
        if ((rc = buf_ensure(c, BUF_BS_H2, sizeof(double) * M * D))) return rc;
        HIPCHK(c, hipMemcpyAsync(buf<double>(c, BUF_BS_H2), h2, sizeof(double) * M * D, hipMemcpyHostToDevice, c->stream));
    }
    PointTables<PostTile> T;
    build_pjvp_tiles(table_classes(P), P.order.data(), offsets, c->posterior_budget, T);
    const size_t Mz = (size_t)std::max<int64_t>(M, 1);
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = buf_ensure(c, BUF_MN_OUT, 2 * Mz * sizeof(double)))) return rc;
    double *d_mean = buf<double>(c, BUF_MN_OUT), *d_var = d_mean + Mz;
    for_solved_chunks(c, P, T, [&](const TileChunk &ch, const SizeClass &k, const MedgpDev &V, const PostTile *tiles) {
        const double *Gk = mc.G + MEAN_PW * k.off_vec, *sk = mc.small + (size_t)k.b0 * mean_small_stride(D), *work = buf<double>(c, BUF_WORK);
        Launcher l(c, basis ? KID_BS_POST : KID_MN_POST);   // (one body, fe_post_body, behind both)
        if (basis) hipLaunchKernelGGL(k_basis_post, dim3(ch.nt), dim3(256), 0, c->stream, V, tiles, buf<int>(c, BUF_META2), buf<double>(c, BUF_BS_H2), work, ch.stride, Gk, sk, mode, D, d_mean, d_var);
        else hipLaunchKernelGGL(k_mean_post, dim3(ch.nt), dim3(256), 0, c->stream, V, tiles, buf<int>(c, BUF_META2), work, ch.stride, Gk, sk, mode, d_mean, d_var);
    });
    HIPCHK(c, hipGetLastError());
    std::vector<double> hs(mc.mb.small_doubles);
    std::vector<int32_t> st(nbatch);
    if ((rc = download_pair<double>(c, M, d_mean, d_var, mean, var))) return rc;
    HIPCHK(c, hipMemcpyAsync(hs.data(), mc.small, mc.mb.small_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_status(c, nbatch, st.data()))) return rc;
    free_retired(c);
    mean_scatter(P, hs, st.data(), nbatch, D, nullptr, beta, nullptr);
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * nbatch);
    return MEDGP_OK;
}

// What the two warp calls share (kernels_warp.h): the argument checks, the plan, the capacity rule, the call's buffers, [psi | zq] and
// kind to the device, ONE pipeline run in the grouped order (factor, U = L^-T; min_n as the caller's family has it) and, per size class
// in stream order, k_warp_z (z = g(y), log g'; a non-finite z: status -1), k_warp_solve (w = U^T z, alpha~ = U w) and k_warp_small
// (1/2 |w|^2, sum log g', dpsi, the objective -> scal[2]).  M, nq: the posterior call's points and quantiles (0, 0: the objective).
struct WarpCall {
    WarpBuffers wb;
    double *vec, *small, *in;
    const int *kind;   // device, or null = all SAS
    int D;
    double *role(int r, size_t need_vec, size_t off_vec) const { return vec + warp_vec_offset(r, need_vec) + off_vec; }
};
int warp_prepare(medgp_ctx *c, const char *who, int nbatch, const int32_t *slots, const double *theta, const int32_t *kind, const double *psi,
                 int min_n, size_t M, int nq, const double *zq, WarpCall &wc) {
    if (!slots || !theta || !psi) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    int rc;
    if ((rc = check_q16(c, who, nullptr))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    const int D = c->rules.D;
    wc.D = D;
    if (kind)
        for (int d = 0; d < D; d++)
            if (kind[d] != MEDGP_WARP_NONE && kind[d] != MEDGP_WARP_SAS) return fail(c, MEDGP_ERR_ARG, "kind[%d] = %d is neither MEDGP_WARP_NONE nor MEDGP_WARP_SAS", d, kind[d]);
    for (size_t i = 0; i < (size_t)nbatch * D * WARP_NPSI; i++)
        if (!std::isfinite(psi[i])) return fail(c, MEDGP_ERR_ARG, "psi[%zu] = %g is not finite", i, psi[i]);
    for (int k = 0; k < nq; k++)
        if (!std::isfinite(zq[k])) return fail(c, MEDGP_ERR_ARG, "zq[%d] = %g is not finite", k, zq[k]);
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = check_one_wave(c, warp_fits(P.need_mat, P.need_vec, c->rules.mem_budget), WARP_MATS, " and vectors"))) return rc;
    wc.wb = warp_buffers(P.need_vec, nbatch, D, M, nq);
    if ((rc = buf_ensure(c, BUF_WP_VEC, wc.wb.vec_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_WP_SMALL, wc.wb.small_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_WP_IN, wc.wb.in_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_WP_KIND, sizeof(int) * D))) return rc;
    wc.vec = buf<double>(c, BUF_WP_VEC); wc.small = buf<double>(c, BUF_WP_SMALL); wc.in = buf<double>(c, BUF_WP_IN);
    wc.kind = kind ? buf<int>(c, BUF_WP_KIND) : nullptr;
    if ((rc = wait_lane0_staging(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(wc.in, psi, sizeof(double) * nbatch * D * WARP_NPSI, hipMemcpyHostToDevice, c->stream));
    if (nq > 0) HIPCHK(c, hipMemcpyAsync(wc.in + warp_in_zq(nbatch, D), zq, sizeof(double) * nq, hipMemcpyHostToDevice, c->stream));
    if (kind) HIPCHK(c, hipMemcpyAsync(buf<int>(c, BUF_WP_KIND), kind, sizeof(int) * D, hipMemcpyHostToDevice, c->stream));
    if ((rc = factor_run_templated(c, nbatch, theta, min_n))) return rc;
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        double *zk = wc.role(WARP_VEC_Z, P.need_vec, k.off_vec), *ljk = wc.role(WARP_VEC_LJ, P.need_vec, k.off_vec);
        double *wk = wc.role(WARP_VEC_W, P.need_vec, k.off_vec), *atk = wc.role(WARP_VEC_AT, P.need_vec, k.off_vec);
        {
            Launcher l(c, KID_WP_Z);
            hipLaunchKernelGGL(k_warp_z, dim3((k.ld + 255) / 256, k.count), dim3(256), 0, c->stream, V, wc.kind, wc.in, zk, ljk);
        }
        {
            Launcher l(c, KID_WP_SOLVE);
            hipLaunchKernelGGL(k_warp_solve, dim3(k.count), dim3(WARP_SOLVE_THREADS), 0, c->stream, V, zk, wk, atk);
        }
        Launcher l(c, KID_WP_SMALL);
        hipLaunchKernelGGL(k_warp_small, dim3(k.count), dim3(256), 0, c->stream, V, wc.kind, wc.in, ljk, wk, atk, wc.small + (size_t)k.b0 * warp_small_stride(D));
    }
    return MEDGP_OK;
}

// The warped nlml and its gradients in theta and psi (kernels_warp.h).  warp_prepare, then per size class in stream order, for a
// gradient: the unchanged k_wgrad on a view whose alpha is alpha~ (W = P - alpha~ alpha~^T tiles -> slab, wdiag); then
// finish_objective_class (k_slabsum, k_epilogue: the objective k_warp_small left in scal[2], to which it adds the priors on theta).
// flag_grad = 0 runs warp_prepare and k_epilogue only.  L and U are never overwritten.
int warp_grad_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int32_t *kind, const double *psi, int flag_grad,
                   double *nlml, double *grad, double *dpsi, double *logjac, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (flag_grad & ~1) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    WarpCall wc{};
    int rc;
    if ((rc = warp_prepare(c, "medgp_warp_nlml_grad", nbatch, slots, theta, kind, psi, 3, 0, 0, nullptr, wc))) return rc;
    const BatchPlan &P = c->plan;
    const int D = wc.D;
    for (const SizeClass &k : P.cls) {
        MedgpDev V = class_view(c, P, k);
        const int nb = k.count;
        V.alpha = wc.role(WARP_VEC_AT, P.need_vec, k.off_vec);   // the gradient pass and what follows see alpha~
        if (flag_grad) {
            Launcher l(c, KID_WGRAD);   // (Q <= 16 was checked)
            launch_wgrad(c, c->stream, V, nb, wgrad_grid(P.en.data() + k.b0, nb, k.nbmax));
        }
        finish_objective_class(c, V, nb, flag_grad);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<double> hs(wc.wb.small_doubles);
    std::vector<int32_t> st(nbatch);
    if ((rc = download_objective(c, nbatch, flag_grad, nlml, grad, st.data(), hs.data(), wc.small, wc.wb.small_doubles * sizeof(double)))) return rc;
    // the per-entry blocks (internal order) to the caller's rows, NaN for failed entries (warp_tables.h: a block's dpsi is laid out
    // [d][k] as the caller's row); an unwarped covariate has no dpsi
    scatter_entry_blocks(P.order.data(), st.data(), nbatch, hs.data(), warp_small_stride(D),
                         {{warp_off_logjac(), 1, logjac}, {warp_off_dpsi(0, 0), (size_t)D * WARP_NPSI, dpsi}});
    for (int b = 0; dpsi && kind && b < nbatch; b++)
        for (int d = 0; d < D && st[b] >= 0; d++)
            if (kind[d] == MEDGP_WARP_NONE) std::fill_n(dpsi + warp_in_psi(b, D, d, 0), WARP_NPSI, 0.0);
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * nbatch);
    return MEDGP_OK;
}

// The warped posterior at test points (kernels_warp.h).  warp_prepare (no n > 2 guard, as medgp_posterior_batch), then per launch chunk
// of tiles of 64 points, in stream order: the unchanged k_pjvp_solve (V = L^-1 K* behind the first panel of every tile's work rows) and
// k_warp_post (zmean, zvar, the quantiles and lpd in fp64).  The points keep the caller's order.
int warp_post_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int32_t *kind, const double *psi,
                   const int64_t *offsets, const int32_t *meta2, const float *t2, const float *y2, int nq, const double *zq, double *zmean,
                   double *zvar, double *quant, double *lpd, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    const char *who = "medgp_warp_posterior_batch";
    if (!offsets) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (nbatch < 1) return fail(c, MEDGP_ERR_CAPACITY, "nbatch %d", nbatch);
    int rc;
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, false, nullptr);   // (zmean / zvar are optional)
    if (M < 0) return (int)M;
    if ((zmean == nullptr) != (zvar == nullptr)) return fail(c, MEDGP_ERR_ARG, "zmean and zvar: both or neither");
    if (nq < 0 || nq > WARP_MAX_NQ) return fail(c, MEDGP_ERR_ARG, "nq = %d outside [0, %d]", nq, WARP_MAX_NQ);
    if (nq > 0 && !zq) return fail(c, MEDGP_ERR_ARG, "zq is NULL with nq = %d", nq);
    if (quant && nq < 1) return fail(c, MEDGP_ERR_ARG, "quant requires nq >= 1 and zq");
    if (lpd && !y2) return fail(c, MEDGP_ERR_ARG, "lpd requires y2");
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, nullptr, ht2, hm2);
    WarpCall wc{};
    if ((rc = warp_prepare(c, who, nbatch, slots, theta, kind, psi, 1, (size_t)M, nq, zq, wc))) return rc;
    const BatchPlan &P = c->plan;
    PointTables<PostTile> T;
    build_pjvp_tiles(table_classes(P), P.order.data(), offsets, c->posterior_budget, T);
    const size_t Mz = (size_t)std::max<int64_t>(M, 1);
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = buf_ensure(c, BUF_WP_OUT, wc.wb.out_doubles * sizeof(double)))) return rc;
    const bool with_y2 = y2 != nullptr && M > 0;
    if (with_y2) {   // (widened once on the host, as the observations are)
        if ((rc = buf_ensure(c, BUF_WP_Y2, Mz * sizeof(double)))) return rc;
        void *pin = nullptr;
        if ((rc = pin_stage(c, sizeof(double) * Mz, &pin))) return rc;
        for (int64_t k = 0; k < M; k++) ((double *)pin)[k] = (double)y2[k];
        HIPCHK(c, hipMemcpyAsync(buf<double>(c, BUF_WP_Y2), pin, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
    }
    double *d_out = buf<double>(c, BUF_WP_OUT);
    double *d_zmean = d_out + warp_out_zmean(Mz), *d_zvar = d_out + warp_out_zvar(Mz), *d_lpd = d_out + warp_out_lpd(Mz), *d_quant = d_out + warp_out_quant(Mz);
    for_solved_chunks(c, P, T, [&](const TileChunk &ch, const SizeClass &k, const MedgpDev &V, const PostTile *tiles) {
        Launcher l(c, KID_WP_POST);
        hipLaunchKernelGGL(k_warp_post, dim3(ch.nt), dim3(256), 0, c->stream, V, tiles, buf<int>(c, BUF_META2), buf<double>(c, BUF_WORK), ch.stride, wc.kind,
                           wc.in, wc.role(WARP_VEC_W, P.need_vec, k.off_vec), with_y2 ? buf<double>(c, BUF_WP_Y2) : (const double *)nullptr, nq,
                           wc.in + warp_in_zq(nbatch, wc.D), d_zmean, d_zvar, d_quant, d_lpd);
    });
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair<double>(c, M, d_zmean, d_zvar, zmean, zvar))) return rc;
    if (M > 0 && quant) HIPCHK(c, hipMemcpyAsync(quant, d_quant, sizeof(double) * M * nq, hipMemcpyDeviceToHost, c->stream));
    if (M > 0 && lpd) HIPCHK(c, hipMemcpyAsync(lpd, d_lpd, sizeof(double) * M, hipMemcpyDeviceToHost, c->stream));
    if ((rc = read_status(c, nbatch, status))) return rc;
    free_retired(c);
    return MEDGP_OK;
}

// ---- the heteroscedastic calls (kernels_hetero.h; geometry: hetero_tables.h; the Student-t constants: robust_tables.h) ---------------
// MedgpDev::nscale is set for the length of ONE call: every way out of it clears the pointer, so no other call ever sees it.
struct HeteroScope {
    medgp_ctx *c;
    explicit HeteroScope(medgp_ctx *c_) : c(c_) {}
    ~HeteroScope() { c->dev.nscale = nullptr; }
};
struct HeteroCall {
    HeteroBuffers hb;
    size_t stride;   // doubles per role of BUF_HT_VEC
    double *vec;
    double *role(int r, const BatchPlan &P, const SizeClass &k) const { return vec + het_vec_offset(r, stride) + P.vec0 + k.off_vec; }
};
// What the three calls share: the argument checks, the plan, the capacity rule, the call's buffers, and the entry table of scales as the
// pointer every class view of the call carries.  M: the posterior call's points; tab_per_entry: doubles of the robust call's table.
int hetero_prepare(medgp_ctx *c, const char *who, int nbatch, const int32_t *slots, const double *theta, size_t M, size_t tab_per_entry, HeteroCall &hc) {
    if (!slots || !theta) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    int rc;
    if ((rc = check_q16(c, who, nullptr))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, false, true))) return rc;
    const BatchPlan &P = c->plan;
    if ((rc = check_one_wave(c, hetero_fits(P.need_mat, P.need_vec, c->rules.mem_budget), HET_MATS, " and vectors"))) return rc;
    hc.stride = het_role_stride(P.vec0, P.need_vec);
    hc.hb = hetero_buffers(P.vec0, P.need_vec, nbatch, M, tab_per_entry);
    if ((rc = buf_ensure(c, BUF_HT_VEC, hc.hb.vec_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_HT_TAB, hc.hb.tab_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_HT_DELTA, hc.hb.delta_doubles * sizeof(double)))) return rc;
    if ((rc = buf_ensure(c, BUF_HT_HAS, sizeof(int) * nbatch))) return rc;
    hc.vec = buf<double>(c, BUF_HT_VEC);
    c->dev.nscale = hc.vec + het_vec_offset(HET_VEC_SCALE, hc.stride);   // (class_view adds the class's offset, as for alpha)
    return wait_lane0_staging(c);
}
// the entry table from the slots' resident scales (use_resident) or all ones
int hetero_load(medgp_ctx *c, const int32_t *slots, int nbatch, bool use_resident, const HeteroCall &hc) {
    const BatchPlan &P = c->plan;
    const double *store = use_resident ? c->d_slot_scale : nullptr;
    if (store) {
        void *pin = nullptr;
        int rc = pin_stage(c, sizeof(int) * nbatch, &pin);
        if (rc) return rc;
        for (int i = 0; i < nbatch; i++) ((int *)pin)[i] = c->h_has_scale[slots[P.order[i]]];
        HIPCHK(c, hipMemcpyAsync(buf<int>(c, BUF_HT_HAS), pin, sizeof(int) * nbatch, hipMemcpyHostToDevice, c->stream));
    }
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        Launcher l(c, KID_HT_LOAD);
        hipLaunchKernelGGL(k_het_load, dim3((k.ld + 255) / 256, k.count), dim3(256), 0, c->stream, V, buf<int>(c, BUF_HT_HAS) + k.b0, store, hc.role(HET_VEC_SCALE, P, k));
    }
    return MEDGP_OK;
}
// k_wgrad (with_w) and k_het_rows on the entries of class k
void hetero_rows(medgp_ctx *c, const BatchPlan &P, const SizeClass &k, const MedgpDev &V, bool with_w, const HeteroCall &hc) {
    if (with_w) {
        Launcher l(c, KID_WGRAD);   // (Q <= 16 was checked)
        launch_wgrad(c, c->stream, V, k.count, wgrad_grid(P.en.data() + k.b0, k.count, k.nbmax));
    }
    Launcher l(c, KID_HT_ROWS);
    hipLaunchKernelGGL(k_het_rows, dim3((k.ld + 255) / 256, k.count), dim3(256), 0, c->stream, V, hc.role(HET_VEC_SCALE, P, k), with_w ? 1 : 0,
                       hc.role(HET_VEC_RESID, P, k), hc.role(HET_VEC_FVAR, P, k));
}
// the per-row outputs on their way home (queued; valid once the stream has been waited for), then het_rows_out lays them out
int hetero_rows_download(medgp_ctx *c, const HeteroCall &hc, std::vector<double> &hv, bool want_scale, bool want_resid, bool want_fvar) {
    hv.resize(hc.hb.vec_doubles);
    const bool want[HET_VECS] = {want_scale, want_resid, want_fvar};
    for (int r = 0; r < HET_VECS; r++)
        if (want[r]) HIPCHK(c, hipMemcpyAsync(hv.data() + het_vec_offset(r, hc.stride), hc.vec + het_vec_offset(r, hc.stride), hc.stride * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return MEDGP_OK;
}
void hetero_rows_out(const medgp_ctx *c, const int32_t *slots, const int32_t *st, int nbatch, const HeteroCall &hc, const std::vector<double> &hv, int role, double *dst) {
    if (!dst) return;
    const BatchPlan &P = c->plan;
    std::vector<int> en(nbatch);
    for (int b = 0; b < nbatch; b++) en[b] = c->h_n[slots[b]];
    const std::vector<int64_t> off = het_row_offsets(en.data(), nbatch);
    for (const SizeClass &k : P.cls)
        for (int j = 0; j < k.count; j++) {
            const int b = P.order[k.b0 + j], s = slots[b];
            het_rows_to_caller(hv.data() + het_vec_offset(role, hc.stride) + P.vec0 + k.off_vec + (size_t)j * k.ld, c->h_perm[s].data(), en[b], st[b] >= 0, dst + off[b]);
        }
}

// The heteroscedastic nlml, its gradient and the row statistics.  hetero_prepare, the entry table from the resident scales, ONE pipeline
// run whose assembly reads the table; then per size class in stream order: the unchanged k_wgrad (a gradient or fvar), k_het_rows,
// k_slabsum and k_epilogue in its nlml mode.
int hetero_grad_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int flag_grad, double *nlml, double *grad,
                     double *resid, double *fvar, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (flag_grad & ~1) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    HeteroScope scope(c);
    HeteroCall hc{};
    int rc;
    if ((rc = hetero_prepare(c, "medgp_hetero_nlml_grad", nbatch, slots, theta, 0, 0, hc))) return rc;
    if ((rc = hetero_load(c, slots, nbatch, true, hc))) return rc;
    if ((rc = factor_run_templated(c, nbatch, theta, 3))) return rc;
    const BatchPlan &P = c->plan;
    const bool with_w = flag_grad || fvar;
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        if (with_w || resid) hetero_rows(c, P, k, V, with_w, hc);
        if (flag_grad) launch_slabsum(c, c->stream, V, k.count);
        launch_epilogue(c, c->stream, V, k.count, c->d_theta, flag_grad, 1, c->d_nlml, c->d_grad, c->d_status_out, EPI_NLML);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<double> hv;
    std::vector<int32_t> st(nbatch);
    if ((rc = hetero_rows_download(c, hc, hv, false, resid != nullptr, fvar != nullptr))) return rc;
    if ((rc = download_objective(c, nbatch, flag_grad, nlml, grad, st.data()))) return rc;
    hetero_rows_out(c, slots, st.data(), nbatch, hc, hv, HET_VEC_RESID, resid);
    hetero_rows_out(c, slots, st.data(), nbatch, hc, hv, HET_VEC_FVAR, fvar);
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * nbatch);
    return MEDGP_OK;
}

// Student-t noise by variational reweighting.  `sweeps` times (pipeline run with the inverse, k_wgrad, k_het_rows, k_het_estep), all
// queued on the stream with no host read-back in between; then the evaluation of J and its gradient at the last scales: pipeline run,
// k_wgrad, k_het_rows, k_het_obj (J -> scal[2]) and finish_objective_class.  That is sweeps + 1 factorisations.
int robust_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const double *nu, int sweeps, const double *scale0,
                int flag_grad, double *obj, double *grad, double *scale, double *resid, double *fvar, double *delta, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (flag_grad & ~1) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    if (!nu) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (sweeps < 0 || sweeps > ROBUST_MAX_SWEEPS) return fail(c, MEDGP_ERR_ARG, "sweeps = %d outside [0, %d]", sweeps, ROBUST_MAX_SWEEPS);
    if (!slots || !theta) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    int rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    const int D = c->rules.D;
    {
        const int64_t bad = robust_first_bad_nu(nu, (int64_t)nbatch * D);
        if (bad >= 0) return fail(c, MEDGP_ERR_ARG, "nu[%lld] = %g is not finite and > 0", (long long)bad, nu[bad]);
    }
    std::vector<int> en(nbatch);
    for (int b = 0; b < nbatch; b++) en[b] = c->h_n[slots[b]];
    const std::vector<int64_t> off = het_row_offsets(en.data(), nbatch);
    if (scale0) {
        const int64_t bad = het_first_bad_scale(scale0, off[nbatch]);
        if (bad >= 0) return fail(c, MEDGP_ERR_ARG, "scale0[%lld] = %g outside [2^-40, 2^40]", (long long)bad, scale0[bad]);
    }
    HeteroScope scope(c);
    HeteroCall hc{};
    if ((rc = hetero_prepare(c, "medgp_robust_nlml_grad", nbatch, slots, theta, 0, (size_t)D * ROBUST_TAB, hc))) return rc;
    const BatchPlan &P = c->plan;
    double *d_tab = buf<double>(c, BUF_HT_TAB), *d_delta = buf<double>(c, BUF_HT_DELTA);
    {
        void *pin = nullptr;
        const size_t bytes = sizeof(double) * nbatch * D * ROBUST_TAB;
        if ((rc = pin_stage(c, bytes, &pin))) return rc;
        robust_fill_table(nu, (int64_t)nbatch * D, (double *)pin);
        HIPCHK(c, hipMemcpyAsync(d_tab, pin, bytes, hipMemcpyHostToDevice, c->stream));
    }
    if (scale0) {   // the caller's rows to the grouped rows of every entry, ones in the padding: one transfer
        void *pin = nullptr;
        if ((rc = pin_stage(c, sizeof(double) * P.need_vec, &pin))) return rc;
        double *img = (double *)pin;
        std::fill_n(img, P.need_vec, 1.0);
        for (const SizeClass &k : P.cls)
            for (int j = 0; j < k.count; j++) {
                const int b = P.order[k.b0 + j];
                het_rows_to_grouped(scale0 + off[b], c->h_perm[slots[b]].data(), en[b], k.ld, img + k.off_vec + (size_t)j * k.ld);
            }
        HIPCHK(c, hipMemcpyAsync(hc.vec + het_vec_offset(HET_VEC_SCALE, hc.stride) + P.vec0, img, sizeof(double) * P.need_vec, hipMemcpyHostToDevice, c->stream));
    } else if ((rc = hetero_load(c, slots, nbatch, false, hc))) return rc;
    for (int it = 0; it < sweeps; it++) {
        if ((rc = factor_run_templated(c, nbatch, theta, 3))) return rc;
        for (const SizeClass &k : P.cls) {
            const MedgpDev V = class_view(c, P, k);
            hetero_rows(c, P, k, V, true, hc);
            Launcher l(c, KID_HT_ESTEP);
            hipLaunchKernelGGL(k_het_estep, dim3(k.count), dim3(256), 0, c->stream, V, d_tab, hc.role(HET_VEC_SCALE, P, k), hc.role(HET_VEC_RESID, P, k),
                               hc.role(HET_VEC_FVAR, P, k), d_delta);
        }
    }
    if ((rc = factor_run_templated(c, nbatch, theta, 3))) return rc;
    const bool with_w = flag_grad || fvar;
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        if (with_w || resid) hetero_rows(c, P, k, V, with_w, hc);
        {
            Launcher l(c, KID_HT_OBJ);
            hipLaunchKernelGGL(k_het_obj, dim3(k.count), dim3(256), 0, c->stream, V, d_tab, hc.role(HET_VEC_SCALE, P, k));
        }
        finish_objective_class(c, V, k.count, flag_grad);
    }
    HIPCHK(c, hipGetLastError());
    std::vector<double> hv, hd(nbatch, 0.0);
    std::vector<int32_t> st(nbatch);
    if ((rc = hetero_rows_download(c, hc, hv, scale != nullptr, resid != nullptr, fvar != nullptr))) return rc;
    if ((rc = download_objective(c, nbatch, flag_grad, obj, grad, st.data(), hd.data(), d_delta, sweeps > 0 ? sizeof(double) * nbatch : 0))) return rc;
    hetero_rows_out(c, slots, st.data(), nbatch, hc, hv, HET_VEC_SCALE, scale);
    hetero_rows_out(c, slots, st.data(), nbatch, hc, hv, HET_VEC_RESID, resid);
    hetero_rows_out(c, slots, st.data(), nbatch, hc, hv, HET_VEC_FVAR, fvar);
    for (int b = 0; delta && b < nbatch; b++) delta[b] = st[b] >= 0 ? hd[b] : std::numeric_limits<double>::quiet_NaN();
    if (status) std::memcpy(status, st.data(), sizeof(int32_t) * nbatch);
    return MEDGP_OK;
}

// The heteroscedastic posterior at test points.  hetero_prepare (no n > 2 guard, as medgp_posterior_batch), the entry table from the
// resident scales, one pipeline run; then per launch chunk of tiles of 64 points, in stream order: the unchanged k_pjvp_solve and
// k_het_post (mean, var in fp64).  The points keep the caller's order.
int hetero_post_impl(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets, const int32_t *meta2,
                     const float *t2, const double *s2, double *mean, double *var, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!offsets) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (nbatch < 1) return fail(c, MEDGP_ERR_CAPACITY, "nbatch %d", nbatch);
    int rc;
    const int64_t M = check_points(c, nbatch, offsets, meta2, t2, false, nullptr);   // (mean / var are optional)
    if (M < 0) return (int)M;
    if ((mean == nullptr) != (var == nullptr)) return fail(c, MEDGP_ERR_ARG, "mean and var: both or neither");
    for (int64_t j = 0; s2 && j < M; j++)
        if (!(std::isfinite(s2[j]) && s2[j] >= 0.0 && s2[j] <= HET_SCALE_MAX)) return fail(c, MEDGP_ERR_ARG, "s2[%lld] = %g outside [0, 2^40]", (long long)j, s2[j]);
    std::vector<double> ht2;
    std::vector<int> hm2;
    stage_points(c, M, meta2, t2, nullptr, ht2, hm2);
    HeteroScope scope(c);
    HeteroCall hc{};
    if ((rc = hetero_prepare(c, "medgp_hetero_posterior_batch", nbatch, slots, theta, (size_t)M, 0, hc))) return rc;
    if ((rc = hetero_load(c, slots, nbatch, true, hc))) return rc;
    if ((rc = factor_run_templated(c, nbatch, theta, 1))) return rc;
    const BatchPlan &P = c->plan;
    PointTables<PostTile> T;
    build_pjvp_tiles(table_classes(P), P.order.data(), offsets, c->posterior_budget, T);
    const size_t Mz = (size_t)std::max<int64_t>(M, 1);
    if ((rc = upload_point_call(c, M, ht2, hm2, T.tiles, T.work_need))) return rc;
    if ((rc = buf_ensure(c, BUF_HT_OUT, hc.hb.out_doubles * sizeof(double)))) return rc;
    double *d_out = buf<double>(c, BUF_HT_OUT);
    double *d_mean = d_out + het_out_mean(Mz), *d_var = d_out + het_out_var(Mz), *d_s2 = d_out + 2 * Mz;
    const bool with_s2 = s2 != nullptr && M > 0;
    if (with_s2) {
        void *pin = nullptr;
        if ((rc = pin_stage(c, sizeof(double) * Mz, &pin))) return rc;
        std::memcpy(pin, s2, sizeof(double) * M);
        HIPCHK(c, hipMemcpyAsync(d_s2, pin, sizeof(double) * M, hipMemcpyHostToDevice, c->stream));
    }
    for_solved_chunks(c, P, T, [&](const TileChunk &ch, const SizeClass &, const MedgpDev &V, const PostTile *tiles) {
        Launcher l(c, KID_HT_POST);
        hipLaunchKernelGGL(k_het_post, dim3(ch.nt), dim3(256), 0, c->stream, V, tiles, buf<int>(c, BUF_META2), buf<double>(c, BUF_WORK), ch.stride,
                           with_s2 ? d_s2 : (const double *)nullptr, d_mean, d_var);
    });
    HIPCHK(c, hipGetLastError());
    if ((rc = download_pair<double>(c, M, d_mean, d_var, mean, var))) return rc;
    if ((rc = read_status(c, nbatch, status))) return rc;
    free_retired(c);
    return MEDGP_OK;
}

}  // namespace

extern "C" {

int medgp_set_noise_scale(medgp_ctx *c, int nslots, const int32_t *slots, const int64_t *offsets, const double *scale) {
    if (!c) return MEDGP_ERR_ARG;
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (nslots < 1 || !slots) return fail(c, MEDGP_ERR_ARG, "medgp_set_noise_scale: bad argument");
    for (int k = 0; k < nslots; k++)
        if (slots[k] < 0 || slots[k] >= c->max_slots || c->h_n[slots[k]] < 0) return fail(c, MEDGP_ERR_ARG, "slots[%d] = %d is not a resident patient", k, slots[k]);
    if (!scale) {   // drop the tables
        for (int k = 0; k < nslots; k++) c->h_has_scale[slots[k]] = 0;
        return MEDGP_OK;
    }
    if (!offsets) return fail(c, MEDGP_ERR_ARG, "offsets is NULL");
    if (offsets[0] != 0) return fail(c, MEDGP_ERR_ARG, "offsets[0] = %lld, expected 0", (long long)offsets[0]);
    for (int k = 0; k < nslots; k++)
        if (offsets[k + 1] - offsets[k] != c->h_n[slots[k]])
            return fail(c, MEDGP_ERR_ARG, "offsets[%d..%d]: %lld scales for the %d observations of slot %d", k, k + 1, (long long)(offsets[k + 1] - offsets[k]), c->h_n[slots[k]], slots[k]);
    {
        const int64_t bad = het_first_bad_scale(scale, offsets[nslots]);
        if (bad >= 0) return fail(c, MEDGP_ERR_ARG, "scale[%lld] = %g outside [2^-40, 2^40]", (long long)bad, scale[bad]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc;
    if (!c->d_slot_scale && (rc = dalloc(c, &c->d_slot_scale, (size_t)c->max_slots * c->ldn))) return rc;
    for (int k = 0; k < nslots; k++) {
        const int s = slots[k], n = c->h_n[s];
        if (n > 0) {
            void *pin = nullptr;
            if ((rc = pin_stage(c, sizeof(double) * n, &pin))) return rc;
            het_rows_to_grouped(scale + offsets[k], c->h_perm[s].data(), n, n, (double *)pin);
            HIPCHK(c, hipMemcpyAsync(c->d_slot_scale + (size_t)s * c->ldn, pin, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        }
    }
    for (int k = 0; k < nslots; k++) c->h_has_scale[slots[k]] = 1;   // (only once every copy is queued: a failure above leaves the call without effect)
    return MEDGP_OK;
}

int medgp_hetero_nlml_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int flag_grad, double *nlml, double *grad,
                           double *resid, double *fvar, int32_t *status) {
    return hetero_grad_impl(c, nbatch, slots, theta, flag_grad, nlml, grad, resid, fvar, status);
}

int medgp_hetero_posterior_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                                 const int32_t *meta2, const float *t2, const double *s2, double *mean, double *var, int32_t *status) {
    return hetero_post_impl(c, nbatch, slots, theta, offsets, meta2, t2, s2, mean, var, status);
}

int medgp_robust_nlml_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const double *nu, int sweeps,
                           const double *scale0, int flag_grad, double *obj, double *grad, double *scale, double *resid, double *fvar,
                           double *delta, int32_t *status) {
    return robust_impl(c, nbatch, slots, theta, nu, sweeps, scale0, flag_grad, obj, grad, scale, resid, fvar, delta, status);
}

int medgp_warp_nlml_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int32_t *kind, const double *psi,
                         int flag_grad, double *nlml, double *grad, double *dpsi, double *logjac, int32_t *status) {
    return warp_grad_impl(c, nbatch, slots, theta, kind, psi, flag_grad, nlml, grad, dpsi, logjac, status);
}

int medgp_warp_posterior_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int32_t *kind, const double *psi,
                               const int64_t *offsets, const int32_t *meta2, const float *t2, const float *y2, int nq, const double *zq,
                               double *zmean, double *zvar, double *quant, double *lpd, int32_t *status) {
    return warp_post_impl(c, nbatch, slots, theta, kind, psi, offsets, meta2, t2, y2, nq, zq, zmean, zvar, quant, lpd, status);
}

int medgp_mean_nlml_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0, const double *lam,
                         int flag_grad, double *nlml, double *grad, double *dmean, double *beta, double *beta_cov, int32_t *status) {
    return mean_grad_impl(c, "medgp_mean_nlml_grad", false, nbatch, slots, theta, mode, b0, lam, flag_grad, nlml, grad, dmean, beta, beta_cov, status);
}

int medgp_mean_posterior_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0,
                               const double *lam, const int64_t *offsets, const int32_t *meta2, const float *t2, double *mean, double *var,
                               double *beta, int32_t *status) {
    return mean_post_impl(c, "medgp_mean_posterior_batch", false, nbatch, slots, theta, mode, b0, lam, offsets, meta2, t2, nullptr, mean, var, beta, status);
}

int medgp_basis_nlml_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0, const double *lam,
                          int flag_grad, double *nlml, double *grad, double *dbeta, double *beta, double *beta_cov, int32_t *status) {
    return mean_grad_impl(c, "medgp_basis_nlml_grad", true, nbatch, slots, theta, mode, b0, lam, flag_grad, nlml, grad, dbeta, beta, beta_cov, status);
}

int medgp_basis_posterior_batch(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0,
                                const double *lam, const int64_t *offsets, const int32_t *meta2, const float *t2, const double *h2,
                                double *mean, double *var, double *beta, int32_t *status) {
    return mean_post_impl(c, "medgp_basis_posterior_batch", true, nbatch, slots, theta, mode, b0, lam, offsets, meta2, t2, h2, mean, var, beta, status);
}

// The resident bases (basis_tables.h).  Everything is validated before any state changes.  The rows of all listed slots are packed in
// the grouped order (the slot's permutation) into one pinned buffer and travel in ONE copy into one contiguous range of the store: in
// place when the call repeats an earlier one, otherwise behind what is used; when the block is too small the live ranges are
// compacted into a new one by device-to-device copies in stream order and the old block is retired (freed at the context's next
// idle point), so nothing here waits for the device unless the pinned buffer of the previous call is still being read.
int medgp_set_basis(medgp_ctx *c, int nslots, const int32_t *slots, int p, const int64_t *offsets, const double *hmat) {
    if (!c) return MEDGP_ERR_ARG;
    if (c->max_slots == 0) return fail(c, MEDGP_ERR_CAPACITY, "call medgp_reserve first");
    if (nslots < 1 || !slots) return fail(c, MEDGP_ERR_ARG, "medgp_set_basis: bad argument");
    std::vector<uint8_t> seen((size_t)c->max_slots, 0);
    for (int k = 0; k < nslots; k++) {
        if (slots[k] < 0 || slots[k] >= c->max_slots) return fail(c, MEDGP_ERR_CAPACITY, "slot %d outside [0, %d)", slots[k], c->max_slots);
        if (seen[slots[k]]) return fail(c, MEDGP_ERR_ARG, "slot %d appears twice in one medgp_set_basis", slots[k]);
        seen[slots[k]] = 1;
    }
    if (!hmat) {   // remove
        for (int k = 0; k < nslots; k++) c->basis.drop(slots[k]);
        return MEDGP_OK;
    }
    if (p < 1) return fail(c, MEDGP_ERR_ARG, "p = %d: a basis has at least one column", p);
    if (p > BASIS_MAX_P) return fail(c, MEDGP_ERR_CAPACITY, "p = %d: a basis has at most %d columns (one 64-column panel)", p, BASIS_MAX_P);
    if (!offsets) return fail(c, MEDGP_ERR_ARG, "offsets is NULL");
    std::vector<int> rows(nslots);
    for (int k = 0; k < nslots; k++) {
        const int n = c->h_n[slots[k]];
        if (n < 0) return fail(c, MEDGP_ERR_ARG, "slot %d holds no patient", slots[k]);
        if (offsets[k + 1] - offsets[k] != n) return fail(c, MEDGP_ERR_ARG, "slot %d: %lld basis rows for a patient of n = %d", slots[k], (long long)(offsets[k + 1] - offsets[k]), n);
        if (offsets[k] < 0) return fail(c, MEDGP_ERR_ARG, "offsets[%d] = %lld", k, (long long)offsets[k]);
        rows[k] = n;
        const double *h = hmat + (size_t)offsets[k] * p;
        for (size_t i = 0; i < (size_t)n * p; i++)
            if (!std::isfinite(h[i])) return fail(c, MEDGP_ERR_ARG, "slot %d: hmat[%zu] = %g is not finite", slots[k], i, h[i]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    size_t total = 0;
    for (int k = 0; k < nslots; k++) total += BasisStore::need(rows[k], p);
    const size_t bytes = std::max<size_t>(total, 1) * sizeof(double);
    if (c->basis_pending) { HIPCHK(c, hipEventSynchronize(c->ev_basis)); c->basis_pending = false; }
    if (bytes > c->basis_stage_cap) {
        AllocTimer tm(c);
        if (c->h_basis_stage) (void)hipHostFree(c->h_basis_stage);
        c->h_basis_stage = nullptr; c->basis_stage_cap = 0;
        HIPCHK(c, hipHostMalloc((void **)&c->h_basis_stage, bytes + bytes / 4, hipHostMallocDefault));
        c->basis_stage_cap = bytes + bytes / 4;
    }
    if (!c->ev_basis) HIPCHK(c, hipEventCreateWithFlags(&c->ev_basis, hipEventDisableTiming));
    const BasisStore before = c->basis;
    const BasisPlace pl = c->basis.place(nslots, slots, rows.data(), p);
    if (pl.new_cap) {
        double *nb = nullptr;
        int rc = dalloc(c, &nb, pl.new_cap);
        if (rc) { c->basis = before; return rc; }
        for (const BasisMove &m : pl.moves)
            HIPCHK(c, hipMemcpyAsync(nb + m.dst, c->d_basis + m.src, m.count * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        if (c->d_basis) {   // queued kernels may still read it
            c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void *)c->d_basis), c->allocs.end());
            c->retired.push_back(c->d_basis);
            c->retired_bytes += before.cap * sizeof(double);
        }
        c->d_basis = nb;
    }
    double *st = (double *)c->h_basis_stage;
    size_t at = 0;
    for (int k = 0; k < nslots; k++) {
        basis_pack_rows(hmat + (size_t)offsets[k] * p, c->h_perm[slots[k]].data(), rows[k], p, st + at);
        at += BasisStore::need(rows[k], p);
    }
    if (total) {
        HIPCHK(c, hipMemcpyAsync(c->d_basis + pl.base, st, total * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_basis, c->stream));
        c->basis_pending = true;
    }
    return MEDGP_OK;
}

// The negative forecast score and its gradient (kernels_forecast_grad.h).  ONE pipeline run in the CALLER's order (as
// medgp_forecast_batch: the history of an observation is a leading block of that order) with U = L^-T, then per size class, in
// stream order: k_fc_vec (var, r, g, e, lpd; then J -> scal[2]), and for a gradient k_fc_t (T = U Mbar into the call's own buffer),
// k_fc_scan (running sums of U diag(z), in place), k_fc_qm (Qm into the dead Kmat block).  T and Qm have their rows at the positions of
// the GROUPED order, so the gradient body runs against the grouped patient copy: once every class has stored its operands, bslot is
// pointed at the grouped slots, and per class k_fc_tables redoes cos / sin for that copy, k_fc_wgrad forms the W_fc tiles -> slab,
// wdiag, and finish_objective_class (k_slabsum, k_epilogue) ends the class.
// flag_grad = 0 runs k_fc_vec and k_epilogue only.  The cached batch selection is dropped at the end: the next call uploads its own
// bslot, and medgp_get_factor is refused (L and U are overwritten).
int medgp_forecast_grad(medgp_ctx *c, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets, const int32_t *prefix,
                        int flag_grad, double *obj, double *grad, int32_t *status) {
    if (!c) return MEDGP_ERR_ARG;
    if (!slots || !theta || !obj) return fail(c, MEDGP_ERR_ARG, "NULL argument");
    if (flag_grad & ~1) return fail(c, MEDGP_ERR_ARG, "unknown bits in flag_grad = %d", flag_grad);
    if (flag_grad && !grad) return fail(c, MEDGP_ERR_ARG, "grad is NULL with flag_grad set");
    int rc;
    if ((rc = check_q16(c, "medgp_forecast_grad", "the generic gradient route keeps W in the buffer that holds Qm here"))) return rc;
    if ((rc = check_call(c, nbatch, slots))) return rc;
    std::vector<int> hn(nbatch);
    for (int b = 0; b < nbatch; b++) hn[b] = c->h_n[slots[b]];
    FcError fe;
    if (!fc_check(nbatch, hn.data(), offsets, prefix, &fe)) {
        if (fe.b < 0) return fail(c, MEDGP_ERR_ARG, "offsets is NULL with a prefix table");
        if (fe.i < 0) return fail(c, MEDGP_ERR_ARG, "patient %d: offsets give it %lld prefix values, it has %lld observations (offsets[0] must be 0)", fe.b, fe.value, fe.expect);
        return fail(c, MEDGP_ERR_ARG, "prefix[%lld] = %lld outside [-1, %lld] (patient %d)", fe.i, fe.value, fe.expect, fe.b);
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = set_batch(c, nbatch, slots, true, true))) return rc;
    const BatchPlan &P = c->plan;
    // the per-entry tables, laid out like the vectors of the plan (class offset, then entry by entry)
    std::vector<int> htab((size_t)FC_TAB_INTS * P.need_vec, 0);
    bool switched = false;   // some entry was factored on its caller-order copy
    for (const SizeClass &k : P.cls)
        for (int e = 0; e < k.count; e++) {
            const int b = P.order[k.b0 + e], s = slots[b];
            const bool ident = c->h_perm_identity[s] != 0;
            switched = switched || !ident;
            fc_fill_entry(hn[b], k.ld, prefix ? prefix + offsets[b] : nullptr, ident ? nullptr : c->h_perm[s].data(),
                          htab.data() + (size_t)FC_TAB_INTS * (k.off_vec + (size_t)e * k.ld));
        }
    if ((rc = buf_ensure(c, BUF_GVEC, 4 * P.need_vec * sizeof(double)))) return rc;
    if (flag_grad && (rc = buf_ensure(c, BUF_FC_T, P.need_mat * sizeof(double)))) return rc;
    if ((rc = upload_table(c, BUF_FC_TAB, htab))) return rc;
    double *gvec = buf<double>(c, BUF_GVEC), *tmat = buf<double>(c, BUF_FC_T);
    const int *dtab = buf<int>(c, BUF_FC_TAB);
    if ((rc = wait_lane0_staging(c))) return rc;
    rc = factor_run_templated(c, nbatch, theta);
    // whatever happens from here on, the next call selects its batch afresh and no factor is on offer
    c->last_nbatch = 0;
    c->last_has_inverse = false;
    if (rc) return rc;
    const double log2pi = std::log(2.0 * c->pi);
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        double *vec = gvec + 4 * k.off_vec;
        const int *tab = dtab + FC_TAB_INTS * k.off_vec;
        const int nb = k.count, nt64 = k.nbmax;
        { Launcher l(c, KID_FC_VEC); hipLaunchKernelGGL(k_fc_vec, dim3(4 * nt64, nb), dim3(256), 0, c->stream, V, vec, tab, 0, log2pi); }
        { Launcher l(c, KID_FC_VEC); hipLaunchKernelGGL(k_fc_vec, dim3(1, nb), dim3(256), 0, c->stream, V, vec, tab, 1, log2pi); }
        if (!flag_grad) continue;
        double *Tm = tmat + k.off_mat;
        { Launcher l(c, KID_FC_T); hipLaunchKernelGGL(k_fc_t, dim3(nt64 * nt64, nb), dim3(WG_THREADS), 0, c->stream, V, Tm, tab, nt64); }
        { Launcher l(c, KID_FC_SCAN); hipLaunchKernelGGL(k_fc_scan, dim3(16 * nt64, nb), dim3(256), 0, c->stream, V, tab); }
        { Launcher l(c, KID_FC_QM); hipLaunchKernelGGL(k_fc_qm, dim3(nt64, 16 * nt64, nb), dim3(256), 0, c->stream, V, Tm, vec, tab); }
    }
    if (flag_grad && switched) {   // every class has stored its operands: the gradient body sees the grouped copies
        void *pin = nullptr;
        if ((rc = pin_stage(c, sizeof(int) * nbatch, &pin))) return rc;
        int *hp = (int *)pin;
        for (int i = 0; i < nbatch; i++) hp[i] = slots[P.order[i]];
        HIPCHK(c, hipMemcpyAsync(c->d_bslot, hp, sizeof(int) * nbatch, hipMemcpyHostToDevice, c->stream));
    }
    for (const SizeClass &k : P.cls) {
        const MedgpDev V = class_view(c, P, k);
        const int nb = k.count, nt64 = k.nbmax;
        if (flag_grad) {
            const int *tab = dtab + FC_TAB_INTS * k.off_vec;
            const double *Tm = tmat + k.off_mat;
            if (switched) { Launcher l(c, KID_FC_TABLES); hipLaunchKernelGGL(k_fc_tables, dim3(nb, (V.Q * V.ldn + PREP_CHUNK - 1) / PREP_CHUNK), dim3(256), 0, c->stream, V); }
            const WgradGrid wg = wgrad_grid(P.en.data() + k.b0, nb, nt64);
            launch_tiles(c, KID_FC_WGRAD, V.Q, wg, [&](auto q, auto q0, dim3 tg, dim3 tb) {
                hipLaunchKernelGGL((k_fc_wgrad<decltype(q)::value, decltype(q0)::value>), tg, tb, 0, c->stream, V, Tm, tab, nb, wg.wg_tiles, wg.nbp);
            });
        }
        finish_objective_class(c, V, nb, flag_grad);
    }
    HIPCHK(c, hipGetLastError());
    return download_objective(c, nbatch, flag_grad, obj, grad, status);
}

#ifdef MEDGP_STAMPS
// diagnostic build only: read (and clear) the phase counters of diag_factor_wave
#ifdef MEDGP_DSTAMPS
extern "C" int medgp_debug_read_diag(unsigned long long *out) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag_dbg), sizeof(z)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_diag_dbg), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif
// diagnostic build only: copy out the stamp words k_cholinv left in the slab of batch entry b
int medgp_debug_read_slab(medgp_ctx *c, int b, void *out, int nbytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->dev.slab + (size_t)b * c->dev.slab_stride, nbytes, hipMemcpyDeviceToHost));
    return 0;
}
int medgp_debug_clear_slab(medgp_ctx *c, int b, int nbytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemset(c->dev.slab + (size_t)b * c->dev.slab_stride, 0, nbytes));
    return 0;
}
int medgp_debug_read_xk(medgp_ctx *c, int b, void *out, int nbytes, int clear) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->dev.xk + (size_t)b * 64 * 64, nbytes, hipMemcpyDeviceToHost));
    if (clear) HIPCHK(c, hipMemset(c->dev.xk + (size_t)b * 64 * 64, 0, nbytes));
    return 0;
}
#endif

int medgp_profile_enable(medgp_ctx *c, int enable) {
    if (!c) return MEDGP_ERR_ARG;
    if (!enable && c->profiling) { int rc = drain_events(c); if (rc) return rc; }
    if (enable) {   // warm the event pool outside any timed region (20 steps x 7 launches x 2 events of a default bench run)
        HIPCHK(c, hipSetDevice(c->device));
        while (c->ev_pool.size() < 512) { hipEvent_t e = nullptr; HIPCHK(c, hipEventCreate(&e)); c->ev_pool.push_back(e); }
    }
    c->profiling = enable != 0;
    c->profile_only = (enable >= 2 && enable - 2 < KID_COUNT) ? enable - 2 : -1;
    return MEDGP_OK;
}
// the table existing callers index is frozen at its 23 entries (include/medgp_hip.h); entries added since are reached through the _all count
int medgp_profile_num_kernels(void) { return KID_FORECAST + 1; }
int medgp_profile_num_kernels_all(void) { return KID_FC_WGRAD + 1; }
int medgp_profile_num_kernels_ext(void) { return KID_EXT_COUNT; }
int medgp_profile_num_kernels_ext2(void) { return KID_EXT2_COUNT; }
int medgp_profile_num_kernels_ext3(void) { return KID_COUNT; }
// (callers hold medgp_profile_kernel_name to "" from medgp_profile_num_kernels_ext2() on: the _ext3 entries have a name call of their own)
const char *medgp_profile_kernel_name(int k) { return (k >= 0 && k < KID_EXT2_COUNT) ? kKernelNames[k] : ""; }
const char *medgp_profile_kernel_name_ext3(int k) { return (k >= 0 && k < KID_COUNT) ? kKernelNames[k] : ""; }
int medgp_profile_read(medgp_ctx *c, int k, double *ms_total, int64_t *launches) {
    if (!c || k < 0 || k >= KID_COUNT) return MEDGP_ERR_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = drain_events(c);
    if (rc) return rc;
    if (ms_total) *ms_total = c->prof_ms[k];
    if (launches) *launches = c->prof_n[k];
    return MEDGP_OK;
}
int medgp_profile_reset(medgp_ctx *c) {
    if (!c) return MEDGP_ERR_ARG;
    int rc = drain_events(c);
    if (rc) return rc;
    for (int k = 0; k < KID_COUNT; k++) { c->prof_ms[k] = 0; c->prof_n[k] = 0; }
    return MEDGP_OK;
}

// ---- cohort statistics (no context: a one-shot call on `device`) ----------------------------------------------------------
int medgp_kde_mode_at(int device, int nseries, const int64_t *off, const int32_t *cnt, const double *data, const int64_t *toff,
                      const int32_t *tcnt, const double *test, int weighted, double *mode, double *bw, int32_t *status, double *kernel_ms);
int medgp_kde_mode(int device, int nseries, const int64_t *off, const int32_t *cnt, const double *data, int weighted,
                   double *mode, double *bw, int32_t *status, double *kernel_ms) {
    return medgp_kde_mode_at(device, nseries, off, cnt, data, nullptr, nullptr, nullptr, weighted, mode, bw, status, kernel_ms);
}
int medgp_kde_mode_at(int device, int nseries, const int64_t *off, const int32_t *cnt, const double *data, const int64_t *toff,
                      const int32_t *tcnt, const double *test, int weighted, double *mode, double *bw, int32_t *status, double *kernel_ms) {
    medgp_ctx *none = nullptr;
    if ((tcnt != nullptr) != (toff != nullptr) || (tcnt != nullptr) != (test != nullptr)) return fail(none, MEDGP_ERR_ARG, "medgp_kde_mode_at: toff, tcnt and test go together");
    if (nseries < 0 || (nseries > 0 && (!off || !cnt || !data || !mode || !status))) return fail(none, MEDGP_ERR_ARG, "medgp_kde_mode: bad argument");
    if (nseries == 0) return MEDGP_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(none, MEDGP_ERR_NODEVICE, "medgp_kde_mode: no GPU (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(none, MEDGP_ERR_ARG, "medgp_kde_mode: device %d of %d", device, ndev);
    int64_t total = 0;
    for (int s = 0; s < nseries; s++) {
        if (cnt[s] < 0 || off[s] < 0) return fail(none, MEDGP_ERR_ARG, "medgp_kde_mode: series %d has a negative size / offset", s);
        if (off[s] + cnt[s] > total) total = off[s] + cnt[s];
    }
    int64_t ttotal = 0;
    int maxnt = 0;
    for (int s = 0; tcnt && s < nseries; s++) {
        if (tcnt[s] < 0 || toff[s] < 0) return fail(none, MEDGP_ERR_ARG, "medgp_kde_mode_at: series %d has a negative grid size / offset", s);
        if (toff[s] + tcnt[s] > ttotal) ttotal = toff[s] + tcnt[s];
        maxnt = tcnt[s] > maxnt ? tcnt[s] : maxnt;
    }
    HIPCHK(none, hipSetDevice(device));
    long long *d_toff = nullptr; int *d_tcnt = nullptr; double *d_test = nullptr;
    long long *d_off = nullptr; int *d_cnt = nullptr, *d_st = nullptr; double *d_x = nullptr, *d_mode = nullptr, *d_bw = nullptr, *d_stats = nullptr, *d_part = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = MEDGP_OK;
    auto chk = [&](hipError_t e, const char *what) { if (e != hipSuccess && rc == MEDGP_OK) rc = fail(none, MEDGP_ERR_HIP, "medgp_kde_mode: %s failed: %s", what, hipGetErrorString(e)); return e == hipSuccess; };
    static_assert(sizeof(long long) == sizeof(int64_t), "offsets are passed through as 64-bit");
    int maxn = 0;
    for (int s = 0; s < nseries; s++) maxn = cnt[s] > maxn ? cnt[s] : maxn;
    const int rankchunks = maxn > 0 ? (maxn + KDE_THREADS - 1) / KDE_THREADS : 1;
    const int maxe = maxn > maxnt ? maxn : maxnt;
    const int maxchunks = maxe > 0 ? (maxe + KDE_THREADS - 1) / KDE_THREADS : 1;
    if (chk(hipMalloc(&d_off, sizeof(long long) * nseries), "hipMalloc") && chk(hipMalloc(&d_cnt, sizeof(int) * nseries), "hipMalloc") &&
        chk(hipMalloc(&d_st, sizeof(int) * nseries), "hipMalloc") && chk(hipMalloc(&d_x, sizeof(double) * (total > 0 ? total : 1)), "hipMalloc") &&
        chk(hipMalloc(&d_mode, sizeof(double) * nseries), "hipMalloc") && chk(hipMalloc(&d_bw, sizeof(double) * nseries), "hipMalloc") &&
        chk(hipMalloc(&d_stats, sizeof(double) * KDE_NSTAT * nseries), "hipMalloc") &&
        chk(hipMalloc(&d_part, sizeof(double) * 4 * (size_t)nseries * maxchunks), "hipMalloc") &&
        chk(hipEventCreate(&e0), "hipEventCreate") && chk(hipEventCreate(&e1), "hipEventCreate") &&
        chk(hipMemcpy(d_off, off, sizeof(long long) * nseries, hipMemcpyHostToDevice), "hipMemcpy") &&
        chk(hipMemcpy(d_cnt, cnt, sizeof(int) * nseries, hipMemcpyHostToDevice), "hipMemcpy") &&
        chk(hipMemcpy(d_x, data, sizeof(double) * total, hipMemcpyHostToDevice), "hipMemcpy") &&
        chk(hipMemset(d_stats, 0, sizeof(double) * KDE_NSTAT * nseries), "hipMemset") &&
        (!tcnt || (chk(hipMalloc(&d_toff, sizeof(long long) * nseries), "hipMalloc") && chk(hipMalloc(&d_tcnt, sizeof(int) * nseries), "hipMalloc") &&
                   chk(hipMalloc(&d_test, sizeof(double) * (ttotal > 0 ? ttotal : 1)), "hipMalloc") &&
                   chk(hipMemcpy(d_toff, toff, sizeof(long long) * nseries, hipMemcpyHostToDevice), "hipMemcpy") &&
                   chk(hipMemcpy(d_tcnt, tcnt, sizeof(int) * nseries, hipMemcpyHostToDevice), "hipMemcpy") &&
                   chk(hipMemcpy(d_test, test, sizeof(double) * ttotal, hipMemcpyHostToDevice), "hipMemcpy")))) {
        chk(hipEventRecord(e0, nullptr), "hipEventRecord");
        hipLaunchKernelGGL(k_kde_stats, dim3(nseries), dim3(KDE_THREADS), 0, nullptr, nseries, d_off, d_cnt, d_x, d_stats);
        hipLaunchKernelGGL(k_kde_rank, dim3(nseries, rankchunks), dim3(KDE_THREADS), 0, nullptr, d_off, d_cnt, d_x, d_stats);
        hipLaunchKernelGGL(k_kde_dens, dim3(nseries, maxchunks), dim3(KDE_THREADS), 0, nullptr, d_off, d_cnt, d_x, d_toff, d_tcnt, d_test, d_stats,
                           d_part, maxchunks);
        hipLaunchKernelGGL(k_kde_final, dim3((nseries + 255) / 256), dim3(256), 0, nullptr, nseries, d_off, d_cnt, d_x, d_toff, d_tcnt, d_test,
                           d_stats, d_part, maxchunks, weighted ? 1 : 0, d_mode, d_bw, d_st);
        chk(hipGetLastError(), "kde kernel launch");
        chk(hipEventRecord(e1, nullptr), "hipEventRecord");
        chk(hipMemcpy(mode, d_mode, sizeof(double) * nseries, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(status, d_st, sizeof(int) * nseries, hipMemcpyDeviceToHost), "hipMemcpy");
        if (bw) chk(hipMemcpy(bw, d_bw, sizeof(double) * nseries, hipMemcpyDeviceToHost), "hipMemcpy");
        if (kernel_ms && rc == MEDGP_OK) { float ms = 0.f; chk(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime"); *kernel_ms = ms; }
        // a non-finite grid point makes the reference's arg-max / weighted mean NaN (np.argmax returns the NaN's index): report
        // the series as failed instead of silently skipping the point
        for (int s = 0; tcnt && rc == MEDGP_OK && s < nseries; s++)
            for (int i = 0; i < tcnt[s]; i++)
                if (!std::isfinite(test[toff[s] + i])) { status[s] = -1; mode[s] = std::nan(""); break; }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    for (void *q : {(void *)d_off, (void *)d_cnt, (void *)d_st, (void *)d_x, (void *)d_mode, (void *)d_bw, (void *)d_stats, (void *)d_part, (void *)d_toff, (void *)d_tcnt, (void *)d_test}) (void)hipFree(q);
    return rc;
}

// ---- kernel clustering: batched EM for Gaussian mixtures (kernels_gmm.h; no context) ---------------------------------------
int medgp_gmm_fit(int device, int n, int d, const double *x, int nruns, const int32_t *k, const int32_t *label0, int max_iter,
                  double tol, double reg_covar, double *lower_bound, double *bic, int32_t *n_iter, int32_t *status,
                  double *weights, double *means, double *covs, int32_t *assign, double *kernel_ms) {
    medgp_ctx *none = nullptr;
    if (!x || !k || !label0 || !lower_bound || !bic || !n_iter || !status) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: NULL argument");
    if (n < 2 || n > INT32_MAX - GMM_BLOCK) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: n = %d, expected at least 2 points", n);
    if (d < 1 || d > MEDGP_GMM_MAX_D) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: d = %d outside [1, %d] (MEDGP_GMM_MAX_D)", d, MEDGP_GMM_MAX_D);
    if (nruns < 1 || nruns > 65535) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: nruns = %d outside [1, 65535]", nruns);
    if (max_iter < 1) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: max_iter = %d, expected >= 1", max_iter);
    if (!(tol >= 0.0) || !(reg_covar >= 0.0)) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: tol = %g / reg_covar = %g, expected >= 0", tol, reg_covar);
    int kmax = 0;
    for (int r = 0; r < nruns; r++) {
        if (k[r] < 1 || k[r] > MEDGP_GMM_MAX_K || k[r] > n)
            return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: k[%d] = %d outside [1, min(%d (MEDGP_GMM_MAX_K), n = %d)]", r, k[r], MEDGP_GMM_MAX_K, n);
        kmax = std::max(kmax, (int)k[r]);
        for (int i = 0; i < n; i++) {
            const int32_t l = label0[(size_t)r * n + i];
            if (l < 0 || l >= k[r]) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: label0[%d, %d] = %d outside [0, %d)", r, i, l, k[r]);
        }
    }
    GmmPlan pl;
    if (!gmm_plan(n, d, nruns, kmax, &pl)) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: sizes outside the supported range");
    double budget_gb = 8.0;
    if (const char *e = getenv("MEDGP_GMM_BUDGET_GB")) { const double v = atof(e); if (v > 0.0) budget_gb = v; }
    if ((double)pl.bytes > budget_gb * 1073741824.0)
        return fail(none, MEDGP_ERR_CAPACITY, "medgp_gmm_fit: %d runs of up to %d components on %d x %d points need %.3f GB at once, the budget is %g GB (MEDGP_GMM_BUDGET_GB): split the runs over calls",
                    nruns, kmax, n, d, (double)pl.bytes / 1073741824.0, budget_gb);
    int poll = 8;
    if (const char *e = getenv("MEDGP_GMM_POLL")) { const int v = atoi(e); if (v >= 1) poll = v; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(none, MEDGP_ERR_NODEVICE, "medgp_gmm_fit: no GPU (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(none, MEDGP_ERR_ARG, "medgp_gmm_fit: device %d of %d", device, ndev);
    HIPCHK(none, hipSetDevice(device));

    // one block: the doubles first, then the ints
    const int64_t rk = (int64_t)nruns * kmax;
    const int64_t nd = pl.x_elems + pl.resp_elems + pl.par_elems + 2 * pl.mat_elems + 3 * rk + pl.blk_elems + pl.lse_elems + pl.sx_elems + pl.slab_elems + 3 * (int64_t)nruns;
    const int64_t ni = pl.label_elems + rk + 3 * (int64_t)nruns;
    char *blockp = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = MEDGP_OK;
    auto chk = [&](hipError_t e, const char *what) { if (e != hipSuccess && rc == MEDGP_OK) rc = fail(none, MEDGP_ERR_HIP, "medgp_gmm_fit: %s failed: %s", what, hipGetErrorString(e)); return e == hipSuccess; };
    std::vector<double> xp((size_t)pl.x_elems, 0.0);
    for (int i = 0; i < n; i++) std::copy(x + (size_t)i * d, x + (size_t)(i + 1) * d, xp.begin() + (size_t)i * pl.dp);
    if (chk(hipMalloc(&blockp, (size_t)(8 * nd + 4 * ni)), "hipMalloc") && chk(hipMemset(blockp, 0, (size_t)(8 * nd + 4 * ni)), "hipMemset") &&
        chk(hipEventCreate(&e0), "hipEventCreate") && chk(hipEventCreate(&e1), "hipEventCreate")) {
        GmmDev G{};
        G.n = n; G.d = d; G.dp = pl.dp; G.nblk = pl.nblk; G.npad = pl.npad; G.bpc = pl.bpc; G.nchunk = pl.nchunk; G.nruns = nruns; G.kmax = kmax;
        G.tol = tol; G.reg = reg_covar;
        double *dptr = (double *)blockp;
        auto take = [&](int64_t cnt) { double *q = dptr; dptr += cnt; return q; };
        double *d_x = take(pl.x_elems);
        G.x = d_x; G.resp = take(pl.resp_elems); G.mu = take(pl.par_elems); G.cov = take(pl.mat_elems); G.P = take(pl.mat_elems);
        G.nk = take(rk); G.logw = take(rk); G.logdet = take(rk); G.blk_nk = take(pl.blk_elems); G.blk_lse = take(pl.lse_elems);
        G.sx = take(pl.sx_elems); G.slab = take(pl.slab_elems); G.lb = take(nruns); G.prev = take(nruns); G.score = take(nruns);
        int *iptr = (int *)dptr;
        auto takei = [&](int64_t cnt) { int *q = iptr; iptr += cnt; return q; };
        int *d_k = takei(nruns);
        G.k = d_k; G.label = takei(pl.label_elems); G.cfail = takei(rk); G.niter = takei(nruns); G.status = takei(nruns);
        std::vector<int32_t> hst(nruns, 0);
        if (chk(hipMemcpy(d_x, xp.data(), sizeof(double) * pl.x_elems, hipMemcpyHostToDevice), "hipMemcpy") &&
            chk(hipMemcpy(d_k, k, sizeof(int) * nruns, hipMemcpyHostToDevice), "hipMemcpy") &&
            chk(hipMemcpy(G.label, label0, sizeof(int) * pl.label_elems, hipMemcpyHostToDevice), "hipMemcpy")) {
            const dim3 g_pts(pl.nblk, kmax, nruns), g_resp(pl.nblk, nruns), g_chunk(pl.nchunk, kmax, nruns), g_comp(kmax, nruns), g_run((nruns + 63) / 64);
            auto mstep = [&]() {
                hipLaunchKernelGGL(k_gmm_msum, g_chunk, dim3(128), 0, nullptr, G);
                hipLaunchKernelGGL(k_gmm_means, g_comp, dim3(128), 0, nullptr, G);
                hipLaunchKernelGGL(k_gmm_cov, g_chunk, dim3(256), 0, nullptr, G);
                hipLaunchKernelGGL(k_gmm_factor, g_comp, dim3(256), 0, nullptr, G);
            };
            chk(hipEventRecord(e0, nullptr), "hipEventRecord");
            hipLaunchKernelGGL(k_gmm_resp, g_resp, dim3(64), 0, nullptr, G, (int)GMM_PHASE_INIT);
            mstep();
            hipLaunchKernelGGL(k_gmm_tail, g_run, dim3(64), 0, nullptr, G, (int)GMM_PHASE_INIT, 0);
            for (int it = 1; it <= max_iter && rc == MEDGP_OK; it++) {
                hipLaunchKernelGGL(k_gmm_estep, g_pts, dim3(256), 0, nullptr, G, (int)GMM_PHASE_ITER);
                hipLaunchKernelGGL(k_gmm_resp, g_resp, dim3(64), 0, nullptr, G, (int)GMM_PHASE_ITER);
                mstep();
                hipLaunchKernelGGL(k_gmm_tail, g_run, dim3(64), 0, nullptr, G, (int)GMM_PHASE_ITER, it);
                if (it % poll == 0 && it < max_iter) {   // the runs freeze on the device: this only decides when the host stops launching
                    if (!chk(hipMemcpy(hst.data(), G.status, sizeof(int) * nruns, hipMemcpyDeviceToHost), "hipMemcpy")) break;
                    if (std::all_of(hst.begin(), hst.end(), [](int32_t s) { return s != GMM_RUNNING; })) break;
                }
            }
            hipLaunchKernelGGL(k_gmm_estep, g_pts, dim3(256), 0, nullptr, G, (int)GMM_PHASE_FINAL);
            hipLaunchKernelGGL(k_gmm_resp, g_resp, dim3(64), 0, nullptr, G, (int)GMM_PHASE_FINAL);
            hipLaunchKernelGGL(k_gmm_tail, g_run, dim3(64), 0, nullptr, G, (int)GMM_PHASE_FINAL, 0);
            chk(hipGetLastError(), "gmm kernel launch");
            chk(hipEventRecord(e1, nullptr), "hipEventRecord");
            std::vector<double> hscore(nruns), hnk((size_t)rk), hmu, hcov;
            chk(hipMemcpy(lower_bound, G.lb, sizeof(double) * nruns, hipMemcpyDeviceToHost), "hipMemcpy");
            chk(hipMemcpy(hscore.data(), G.score, sizeof(double) * nruns, hipMemcpyDeviceToHost), "hipMemcpy");
            chk(hipMemcpy(n_iter, G.niter, sizeof(int) * nruns, hipMemcpyDeviceToHost), "hipMemcpy");
            chk(hipMemcpy(status, G.status, sizeof(int) * nruns, hipMemcpyDeviceToHost), "hipMemcpy");
            if (weights) chk(hipMemcpy(hnk.data(), G.nk, sizeof(double) * rk, hipMemcpyDeviceToHost), "hipMemcpy");
            if (means) { hmu.resize((size_t)pl.par_elems); chk(hipMemcpy(hmu.data(), G.mu, sizeof(double) * pl.par_elems, hipMemcpyDeviceToHost), "hipMemcpy"); }
            if (covs) { hcov.resize((size_t)pl.mat_elems); chk(hipMemcpy(hcov.data(), G.cov, sizeof(double) * pl.mat_elems, hipMemcpyDeviceToHost), "hipMemcpy"); }
            if (assign) chk(hipMemcpy(assign, G.label, sizeof(int) * pl.label_elems, hipMemcpyDeviceToHost), "hipMemcpy");
            if (kernel_ms && rc == MEDGP_OK) { float ms = 0.f; chk(hipEventElapsedTime(&ms, e0, e1), "hipEventElapsedTime"); *kernel_ms = ms; }
            const double qnan = std::nan("");
            for (int r = 0; rc == MEDGP_OK && r < nruns; r++) {
                const bool ok = status[r] != GMM_FAILED;
                const int K = k[r];
                // free parameters of a full-covariance mixture: K d (d + 1) / 2 + K d + K - 1
                const double npar = (double)K * d * (d + 1) / 2.0 + (double)K * d + K - 1;
                if (!ok) lower_bound[r] = qnan;
                bic[r] = ok ? -2.0 * hscore[r] * n + npar * std::log((double)n) : qnan;
                for (int c = 0; c < kmax; c++) {
                    const size_t q = (size_t)r * kmax + c;
                    const bool in = c < K;
                    if (weights) weights[q] = !in ? 0.0 : ok ? hnk[q] / n : qnan;
                    for (int j = 0; means && j < d; j++) means[q * d + j] = !in ? 0.0 : ok ? hmu[q * pl.dp + j] : qnan;
                    for (int i = 0; covs && i < d; i++)
                        for (int j = 0; j < d; j++) covs[(q * d + i) * d + j] = !in ? 0.0 : ok ? hcov[(q * pl.dp + i) * pl.dp + j] : qnan;
                }
                for (int i = 0; assign && !ok && i < n; i++) assign[(size_t)r * n + i] = -1;
            }
        }
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(blockp);
    return rc;
}

}  // extern "C"
