/*
 * medgp_hip.h -- C ABI of the MI355X-native MedGP hot path (libmedgp_hip.so).
 *
 * This is the drop-in boundary for the per-patient negative-log-marginal-likelihood + gradient
 * operator of bee-hive/MedGP.  Every entry point cites the reference interface it replaces
 * ("ref:" = /root/reference/medgpc/src/...).  Plain pointers and sizes only; no C++ or torch types;
 * never throws, never exit()s; 0 = success, negative = error (message via medgp_last_error).
 *
 * Threading: one medgp_ctx is used by one host thread at a time (the reference's callers are
 * single-threaded, ref: inference/c_inference_exact.cpp:55-57); different contexts (e.g. one per GPU)
 * are fully independent and may run concurrently.
 *
 * Hyper-parameter vector theta (doubles, the reference's optimiser variables, ref:
 * core/c_hyperparam.cpp:99-122, kernel/c_kernel_LMC_SM.cpp:51-70):
 *   kernel_index 7 (LMC-SM): [log sigma_d (D) | A_q[d][r] raw, q-major (Q*D*R) | log mu_q (Q) | log v_q (Q) | log kappa_q[d] (Q*D)]
 *   kernel_index 8 (SM)    : [log sigma | log w_q (Q) | log mu_q (Q) | log v_q (Q)]      (D = 1)
 *   kernel_index 0 (SE)    : [log sigma | log l | log sf]                                   (Q = D = 1)
 * Gradients come back in the same order.
 */
#ifndef MEDGP_HIP_H
#define MEDGP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct medgp_ctx medgp_ctx;

/* kernel_index values: ref main_one_train.cpp:85-93 */
#define MEDGP_KERNEL_SE      0
#define MEDGP_KERNEL_LMC_SM  7
#define MEDGP_KERNEL_SM      8

/* error codes */
#define MEDGP_OK            0
#define MEDGP_ERR_ARG      -1   /* bad argument                                   */
#define MEDGP_ERR_HIP      -2   /* a HIP runtime call failed                      */
#define MEDGP_ERR_NODEVICE -3   /* no usable GPU: the product has NO CPU fallback */
#define MEDGP_ERR_CAPACITY -4   /* slot / batch / n beyond medgp_reserve          */

/* prior type codes, ref: prior/c_prior.h:50-53 */
#define MEDGP_PRIOR_NONE    -1
#define MEDGP_PRIOR_CLAMP    0
#define MEDGP_PRIOR_NORMAL   1
#define MEDGP_PRIOR_LAPLACE  2

/* flag_grad bits of medgp_nlml_grad / medgp_nlml_grad_device.  The reference passes a bool (`flag_grad`,
 * ref: inference/c_inference.h:38-52); 0 and 1 keep that meaning.  Bit 1 asks for the factor outputs of the same call
 * (chol_alpha / chol_factor_inv / beta, ref: inference/c_inference_exact.cpp:124-147) to be formed even when no gradient
 * is wanted -- GP_Regression::train(false) followed by GP_Regression::predict, ref: core/gp_regression.cpp:102-214,
 * caller main_one_test.cpp:386-399 -- so that medgp_get_factor is valid afterwards. */
#define MEDGP_FLAG_GRAD        1
#define MEDGP_FLAG_KEEP_FACTOR 2

/* ABI version, bumped on any signature change */
int medgp_abi_version(void);   /* 23: medgp_set_noise_scale, medgp_hetero_nlml_grad, medgp_hetero_posterior_batch, medgp_robust_nlml_grad, medgp_profile_num_kernels_ext3, medgp_profile_kernel_name_ext3 (22: medgp_warp_nlml_grad, medgp_warp_posterior_batch, medgp_profile_num_kernels_ext2; 21:medgp_set_basis, medgp_basis_nlml_grad, medgp_basis_posterior_batch; 20: medgp_mean_nlml_grad, medgp_mean_posterior_batch; 19: medgp_posterior_vjp_batch, medgp_posterior_vjp_moments; 18: medgp_posterior_jvp_batch; 17: medgp_hess_vec; 16: medgp_fisher_vec; 15: medgp_lgo_grad; 14: medgp_forecast_grad; 13: medgp_gmm_fit; 12: medgp_functional_joint_batch; 11: medgp_functional_batch; 10: medgp_components_batch; 9: medgp_trend_batch; 8: medgp_forecast_batch; 7: medgp_loo_grad; 6: medgp_loo_batch; 5: medgp_posterior_joint_batch; 4: medgp_posterior_batch; 3: medgp_reserve_plan, medgp_alloc_stats) */

/* number of visible HIP devices (0 if none; never initialises a context) */
int medgp_device_count(void);

/* Create a context bound to one device and one covariance family.
 * Replaces the construction of c_kernel_* / c_likelihood_* / c_inference_* objects,
 * ref: main_one_train.cpp:103-152 (run_model_LMC_SM / run_model_SE / run_model_SM).
 * R is ignored for SE/SM. */
int  medgp_create(medgp_ctx **out, int device, int kernel_index, int Q, int D, int R);
void medgp_destroy(medgp_ctx *ctx);
const char *medgp_last_error(const medgp_ctx *ctx);   /* ctx may be NULL: last create() error */

/* total number of hypers H = lik + cov (ref: c_kernel_LMC_SM.cpp:64-70; gaussianMO: D) */
int medgp_num_hyp(const medgp_ctx *ctx);

/* pi used inside the kernels; default 3.14159265, the reference's literal
 * (ref: util/global_settings.h:6) */
int medgp_set_pi(medgp_ctx *ctx, double pi);

/* Run all work of this context on the given hipStream_t (e.g. torch's current stream).
 * NULL = the context's own stream (default). */
int medgp_set_stream(medgp_ctx *ctx, void *hip_stream);

/* (Re)allocate device storage: patient slots, largest padded n, largest batch per call.
 * Replaces the per-evaluation new[]/delete[] of N*N buffers, ref: core/gp_regression.cpp:102-117,
 * inference/c_inference_exact.cpp:66-68,168. Existing patients are discarded.
 * The per-entry matrices (two padded n x n fp64 matrices per batch entry) are allocated here when max_batch x max_n^2 of them stay
 * below 8 GB; beyond that (a cohort whose largest patient is far above the rest) they are sized once by medgp_reserve_plan from the
 * patients' sizes, or grown by the calls to what their size classes need (see medgp_last_plan) -- a call that outgrows a buffer replaces
 * it without waiting for anything (the old block is released at the context's next idle point) and drops the factors of earlier calls.  A call whose matrices exceed the memory budget (64 GB, at most 70 % of what the device has free;
 * MEDGP_MEM_BUDGET_GB) is run as consecutive waves of size classes that reuse the arenas; calls whose OUTPUTS need every entry's matrix
 * afterwards (MEDGP_FLAG_KEEP_FACTOR, medgp_factor_batch, medgp_fit_predict_batch) fail with MEDGP_ERR_CAPACITY instead. */
int medgp_reserve(medgp_ctx *ctx, int max_slots, int max_n, int max_batch);

/* Announce the sizes of the patients that will be resident together (n[count] observation counts, any order) and the width of the
 * random-initialisation screening (ninit hyper vectors per patient, 0 = none): the per-entry arenas are mapped ONCE to the high-water
 * mark of (a) one nlml + gradient call over them and (b) the chunks medgp_screen forms of them, so that no later call has to obtain
 * device memory.  Optional -- without it the buffers grow with the calls -- but on this platform obtaining memory that an earlier
 * process has used can take seconds (the driver wipes it first; 0.27 s per GB was measured), and a long-lived trainer wants that wait
 * once, before its loop, not inside it, and for as few bytes as its calls really need.  A cohort host has the sizes before its first call: the reference's
 * job generator reads them to bucket patients by N (ref: medgpc/util/run_exp_generator.py:213-260, scripts/slurm_della.json:6-62),
 * medgp_train takes them from its patient list.  Replaces nothing the reference allocates ahead: it news / deletes its N x N buffers
 * per evaluation (ref: core/gp_regression.cpp:102-117, inference/c_inference_exact.cpp:66-68,168). */
int medgp_reserve_plan(medgp_ctx *ctx, int count, const int32_t *n, int ninit);

/* Memory-management accounting of the context: wall seconds spent obtaining / releasing device memory so far, the number of such
 * calls, and the bytes the per-entry buffers (arenas) hold at present.  Any pointer may be NULL.  (bench.py and medgp_train report it as
 * `alloc_s`: time the host spent waiting for memory instead of queueing work.) */
int medgp_alloc_stats(const medgp_ctx *ctx, double *seconds, int64_t *calls, int64_t *arena_bytes);

/* Upload one patient (meta[i] in [0,D), t = time stamps, y = z-scored values; host pointers, copied).
 * Replaces c_objective_one's constructor, ref: util/c_objective_one.cpp:23-36 and
 * util/c_objective_one.h:40-45.  meta may be NULL for SE/SM.  Observations are stably grouped
 * by output internally (the reference's loader already produces that order,
 * ref: dataio/c_experiment.cpp:272-308), which leaves nlml/gradients unchanged.
 * Supported range of the time stamps: |t| <= 2^14 = 16384 (hours).  The covariance depends on differences only, but the pair
 * kernels form cos(w (t_i - t_j)) from per-observation tables cos(w t_i), sin(w t_i), whose error grows with |w t|: up to 2^14 h
 * nlml and gradient stay inside the fp64 error budget of the test suite for periods down to one hour (measured error at 2^14 h,
 * period 1 h: nlml 1.1e-12, gradient 8.4e-11 relative); at 2^17 h they leave it (5.8e-12 / 3.6e-10).  A caller whose clock
 * starts elsewhere subtracts a per-patient origin (exact for float inputs on a common grid) from t and from the test times.
 * The bound is NOT checked: medgp_set_patient accepts any t.  It was measured on two patients (n = 60, 120) at periods of 1, 12 and
 * 72 h, where the device used half of the nlml budget at 2^14 h; the loss is |w t| eps with w = 2 PI / period, so the range
 * shrinks in proportion for periods under one hour (period 0.25 h: |t| <= 2^12 h). */
int medgp_set_patient(medgp_ctx *ctx, int slot, int n, const int32_t *meta, const float *t, const float *y);

/* Packed upload of nslots patients in ONE host-to-device transfer and without waiting for the device: patient k goes to
 * slots[k] and owns elements [offsets[k], offsets[k+1]) of meta / t / y (offsets has nslots + 1 entries).
 * Replaces a loop of c_objective_one constructions over a cohort, ref: util/c_objective_one.cpp:23-36, the stacked
 * per-feature loader arrays of dataio/c_experiment.cpp:254-309, and the per-(time stamp, observation) training subsets
 * of the imputation loop, ref: main_one_test.cpp:352-365. */
int medgp_set_patients(medgp_ctx *ctx, int nslots, const int32_t *slots, const int64_t *offsets, const int32_t *meta,
                       const float *t, const float *y);

/* Per-hyper prior descriptor of one slot, H entries each in theta order; flag == NULL removes the prior.
 * Replaces the public vectors of c_prior read by c_inference_prior::compute_nlml,
 * ref: prior/c_prior.h:35-53, inference/c_inference_prior.cpp:60-150.
 * slot = -1 applies the descriptor to every slot. */
int medgp_set_prior(medgp_ctx *ctx, int slot, const uint8_t *flag, const int32_t *type,
                    const uint8_t *is_exp, const float *p0, const float *p1);

/* The same for nslots slots in ONE host-to-device transfer and without waiting for the device: row k of the [nslots][H] arrays
 * describes slot slots[k] (flag == NULL removes the prior of all of them).  This is what a cohort trainer calls once per
 * variational-EM outer iteration for every patient whose psi changed -- the reference rebuilds the public vectors of one
 * c_prior object per patient there, ref: util/c_optimizer_varEM.cpp:98-162, prior/c_prior.cpp:222-279. */
int medgp_set_priors(medgp_ctx *ctx, int nslots, const int32_t *slots, const uint8_t *flag, const int32_t *type,
                     const uint8_t *is_exp, const float *p0, const float *p1);

/* THE OPERATOR.  nbatch independent evaluations: problem b = patient slots[b] with hypers
 * theta[b*H .. (b+1)*H).  Replaces c_objective_one::compute_objective -> GP_Regression::train ->
 * c_inference_prior::compute_nlml -> c_inference_exact::compute_nlml,
 * ref: util/c_objective_one.cpp:40-82, core/gp_regression.cpp:102-126,
 *      inference/c_inference_prior.cpp:25-154, inference/c_inference_exact.cpp:29-244,
 *      kernel/c_kernel_LMC_SM.cpp:152-327.
 * flag_grad: 0 = nlml only, MEDGP_FLAG_GRAD = nlml + gradient, | MEDGP_FLAG_KEEP_FACTOR = also keep alpha / L^-1.
 * status[b]: 0..10 = jitter rounds applied (ref: c_inference_exact.cpp:96-111); -1 = the
 * reference's `return false` (Cholesky failed after 10 jitters, or n <= 2,
 * ref: util/c_objective_one.cpp:51,79-81); nlml/grad of a failed problem are NaN.
 * All pointers are HOST memory; grad may be NULL when flag_grad == 0. */
int medgp_nlml_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int flag_grad,
                    double *nlml, double *grad, int32_t *status);

/* Random-initialisation screening: HOT LOOP A of the reference (ref: main_one_train.cpp:228-253 -- every one of the
 * random_init_num hyper vectors evaluated on the patient, nlml only, the smallest wins).  The ninit vectors theta[ninit][H] are the same
 * for every patient (c_experiment::get_global_hyp draws them once from the seed, ref: dataio/c_experiment.cpp:418-441), so they
 * travel to the device ONCE per call and every (patient, vector) entry reads its row there; the nslots * ninit evaluations are
 * queued in calls of at most max_batch entries without a host wait in between.  nlml / status: [nslots][ninit], host memory
 * (status may be NULL).  Each evaluation is bit-identical to medgp_nlml_grad(flag_grad = 0) on the same (patient, vector) in a batch
 * of the same composition. */
int medgp_screen(medgp_ctx *ctx, int nslots, const int32_t *slots, int ninit, const double *theta, double *nlml, int32_t *status);

/* Same operator with theta / nlml / grad / status in DEVICE memory of ctx's device, queued on the context's stream
 * (slots stays a host array: it only selects resident patients; it is copied before the call returns).  Asynchronous for
 * EVERY route: the one-workgroup-per-patient kernel runs the reference's jitter loop (ref: inference/c_inference_exact.cpp:
 * 99-111) in-kernel, and the multi-CU schedule used for few, large entries (at most 0.6 x #CU entries with n > 64) hands the
 * entries whose single attempt failed to that same in-kernel loop on the device (k_cholinv, sel = 2) -- the host reads no
 * status back, and a call that has to grow a buffer waits for nothing either (round 6: the outgrown block is released at the
 * context's next idle point). */
int medgp_nlml_grad_device(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta_dev,
                           int flag_grad, double *nlml_dev, double *grad_dev, int32_t *status_dev);

/* Asynchronous form of medgp_nlml_grad for hosts that overlap their own work (the optimiser state machines of the patients of
 * one half of a cohort, ref: util/c_optimizer_scg.cpp:87-281) with the device working on the other half: the call queues the
 * theta upload, the evaluation and the result downloads of `lane` (0 or 1; each lane has its own device staging) on the context's
 * stream and returns; medgp_wait(ctx, lane) blocks until that lane's results are in nlml / grad / status.  The host arrays must
 * stay valid (and untouched) until then, and overlap needs them in pinned memory: medgp_host_alloc / medgp_host_free
 * (hipHostMalloc; pageable memory works but makes the copies synchronous).  A lane holds one call at a time. */
void *medgp_host_alloc(size_t bytes);
void  medgp_host_free(void *p);
int   medgp_nlml_grad_async(medgp_ctx *ctx, int lane, int nbatch, const int32_t *slots, const double *theta, int flag_grad,
                            double *nlml, double *grad, int32_t *status);
int   medgp_wait(medgp_ctx *ctx, int lane);

/* After medgp_nlml_grad*(…, flag_grad with MEDGP_FLAG_GRAD or MEDGP_FLAG_KEEP_FACTOR): copy out K^-1 (y - m), L^-1 and
 * beta = (y - m)^T K^-1 (y - m) of batch entry b as the reference's float buffers (alpha[n]; linv[n*n] row-major lower,
 * strict upper zero), ALWAYS in the caller's original observation order -- L^-1 is the inverse Cholesky factor of the
 * Gram matrix in that order, exactly what GP_Regression::predict multiplies the caller-order cross Gram with
 * (ref: core/gp_regression.cpp:181-196).  If the entry was evaluated in the internal grouped order (gradient calls on
 * patients not uploaded grouped by output), asking for linv re-factors that one entry in the caller's order.
 * Fails (MEDGP_ERR_ARG) when the last call formed no factor (flag_grad == 0, or medgp_fit_predict*).
 * Replaces the chol_alpha / chol_factor_inv / beta outputs of c_inference::compute_nlml,
 * ref: inference/c_inference.h:38-52, inference/c_inference_exact.cpp:124-147. Any pointer may be NULL. */
int medgp_get_factor(medgp_ctx *ctx, int b, float *alpha, float *linv, float *beta);

/* Factor once with theta, predict nstar points.  Replaces GP_Regression::train(false) + predict,
 * ref: core/gp_regression.cpp:128-214, kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram), :122-150 (diag);
 * caller: main_one_test.cpp:386-399.  mean/var are float like the reference. */
int medgp_fit_predict(medgp_ctx *ctx, int slot, const double *theta, int nstar, const int32_t *meta2,
                      const float *t2, float *mean, float *var, int32_t *status);

/* Cholesky factor of one patient's Gram matrix and z = L^-1 (y - m), fp64, in the CALLER's observation order:
 * L [n*n] row-major lower (strict upper zero), z [n]; either may be NULL.  This is the state LAPACKE_spotrf + the first
 * half of spotrs leave inside c_inference_exact::compute_nlml (ref: inference/c_inference_exact.cpp:96-125) before it is
 * turned into chol_alpha / chol_factor_inv.  It is what the online imputation loop can SHARE between its problems: with the
 * observations in time order every training subset `past(t)` of main_one_test.cpp:287-300 is a leading block of one
 * factorisation (L[0:p, 0:p] is the factor of the first p observations, z[0:p] their solve), and the same-time observations
 * appended at :358-365 are the next rows -- medgp_test's no-update pass does one medgp_factor per patient instead of one
 * factorisation per imputed observation.  status as medgp_nlml_grad (no n > 2 guard, like GP_Regression::train). */
int medgp_factor(medgp_ctx *ctx, int slot, const double *theta, double *L, double *z, int32_t *status);
/* The same for nbatch patients in ONE call (one pipeline run, one read-back): entry b uses patient slots[b] and hypers
 * theta[b*H ..); L[b] receives n_b*n_b doubles, z[b] n_b doubles (either array, or single entries, may be NULL); status[nbatch].
 * What the cohort form of the no-update imputation pass uses (medgp_test --pan-list: one shared factorisation per patient, all
 * patients of a chunk in one call; ref: main_one_test.cpp:287-300, :358-365, :386-399). */
int medgp_factor_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, double *const *L, double *const *z,
                       int32_t *status);

/* nbatch independent (train(false) + predict ONE point) problems in one call: problem b uses patient
 * slots[b], hypers theta[b*H..), test point (meta2[b], t2[b]).  This is the inner body of the online
 * imputation loop, ref: main_one_test.cpp:352-409 (N* = 1 there, :369-372), batched over the (time stamp,
 * observation) pairs of a patient, each uploaded as its own slot (a subset of the patient's observations). */
int medgp_fit_predict_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta,
                            const int32_t *meta2, const float *t2, float *mean, float *var, int32_t *status);

/* Batched posterior with the per-covariate decomposition of the mean.  nbatch patients, patient b = slots[b] with hypers
 * theta[b*H..), test points offsets[b] .. offsets[b+1) of meta2 / t2 (offsets has nbatch + 1 entries, offsets[0] == 0,
 * non-decreasing; an empty range is allowed).  For every test point j: mean[j], var[j] as GP_Regression::predict, and
 * (parts != NULL) parts[j*D + d] = the part of mean[j] carried by the training observations of covariate d, as
 * GP_Regression::parsed_predict (zero mean function: the D parts of a point sum to its mean; D = 1 for SE / SM).
 *   ref: core/gp_regression.cpp:216-320 (parsed_predict), :128-214 (predict),
 *        kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram), :122-150 (self diagonal)
 * status[b] as medgp_fit_predict_batch; the points of a patient with status < 0 get NaN mean, var and parts.  One factorisation
 * per patient, then the points in tiles of 64 per workgroup (forward solve on fp64 MFMA).  A point's outputs do not depend on
 * the other points of the call, their order, or how the call is cut into launches (work memory per launch:
 * MEDGP_POSTERIOR_BUDGET_GB, default 2).  meta2 may be NULL for SE / SM.  Like medgp_fit_predict_batch, a call whose
 * per-entry matrices exceed the memory budget fails with MEDGP_ERR_CAPACITY.
 * Supported range of the time stamps: |t| <= 2^14 h, of the training observations (medgp_set_patient) AND of the test points: for
 * Q <= 8 K* is formed from tables cos / sin (w t_i) and cos / sin (w t*), cos(w (t_i - t*)) = cs_i cc + sn_i sc, whose error grows
 * as |w t| eps.  Up to that limit, at periods down to one hour, mean, var and parts stay within the project's bar of 2 fp32 ulps
 * of max(|ref|, 1e-3 S) of the posterior of the unshifted patient (tests/test_time_shift_gpu.py, at -2^14, 2^10 and 2^14 h).
 * All pointers are HOST memory. */
int medgp_posterior_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                          const int32_t *meta2, const float *t2, float *mean, float *var, float *parts, int32_t *status);

/* Joint posterior of every patient's test points: the covariance of the predictive distribution and sample paths from it.
 * nbatch, slots, theta, offsets, meta2, t2, mean, var, status exactly as medgp_posterior_batch (mean and var are that call's,
 * bit for bit: the same code path).  With m_b = offsets[b+1] - offsets[b]:
 *   cov     (may be NULL) patient b's block starts at cov + sum_{a<b} m_a^2: m_b x m_b, row-major,
 *             C = K** - V^T V + diag(sigma^2_{meta2}),  V = L^-1 K*,
 *           the predictive covariance of y* (noise included, once: diag(C) is `var`, as GP_Regression::predict adds it,
 *           ref: core/gp_regression.cpp:128-214); both triangles written, exactly symmetric.
 *   eps     nsamp standard normals per test point SUPPLIED BY THE CALLER, eps[(offsets[b] + i)*nsamp + s] (the library draws
 *           nothing: a call depends on its arguments alone)
 *   samples same layout, float: samples[(offsets[b] + i)*nsamp + s] = mean_i + sum_{j<=i} Lc[i][j] eps[j][s], Lc the lower
 *           Cholesky factor of C in the caller's order of the points: sample path s of patient b, consistent across times
 *           and covariates.
 * nsamp == 0 (eps, samples NULL): covariance only, C is not factored.  cov == NULL: samples only.  Neither: MEDGP_ERR_ARG.
 * cov_status[b] (may be NULL): 0 ok; -1 the factorisation of C met a pivot <= 0 or NaN (LAPACK's rule; there is no jitter
 * loop, C >= sigma^2_min I in exact arithmetic): that patient's samples are NaN, its cov is still written; also -1 for a
 * patient with status[b] < 0, whose outputs are all NaN.  m_b == 0 is allowed.  A patient's outputs do not depend on the other
 * patients of the call, their order, or how the call is cut into launches.  The reference has no such output (its predict
 * returns marginals); the definition is the fp64 restatement of tests/posterior_joint_ref.py.
 * Memory: V of all tiles of a patient (ld x m_b doubles), C (m_b rounded up to 64, squared, doubles) and its float block are
 * resident together; the call is cut into launches of whole patients within MEDGP_POSTERIOR_BUDGET_GB (default 2), a single
 * patient beyond it fails with MEDGP_ERR_CAPACITY, as does a call whose per-entry matrices exceed the memory budget.  C is
 * factored by one workgroup per patient: made for cohorts of patients with up to a few thousand points each.
 * Supported range of the time stamps: |t| <= 2^14 h, of the training observations AND of the test points, as medgp_posterior_batch:
 * for Q <= 8 K** too is formed from cos / sin (w t*) tables of the test points.  cov and samples are held to the 2-ulp bar at that
 * limit (tests/test_time_shift_gpu.py).
 * All pointers are HOST memory. */
int medgp_posterior_joint_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                                const int32_t *meta2, const float *t2, int nsamp, const double *eps, float *mean, float *var,
                                float *cov, float *samples, int32_t *status, int32_t *cov_status);

/* Leave-one-out / leave-group-out predictive distribution of the TRAINING observations: how well the fitted model predicts the
 * data it was fitted to, without a refit.  The reference has no such output; the definition is the refit restated in
 * tests/loo_ref.py.  With U = L^-T and alpha = K^-1 y of the one factorisation per patient and, for a held-out index set B,
 * M = (K^-1)_BB = U_B U_B^T:
 *   cov(y_B | rest) = M^-1,  mean(y_B | rest) = y_B - M^-1 alpha_B,
 *   log p(y_B | rest) = -1/2 alpha_B^T M^-1 alpha_B + 1/2 log det M - |B|/2 log 2 pi      (Rasmussen & Williams 5.4.2 for |B| = 1).
 * nbatch, slots, theta, status as medgp_posterior_batch (one factorisation per patient, no n > 2 guard; status[b] = jitter rounds
 * or -1).  With n_b the observation count of slots[b], the per-observation arrays are concatenated by patient in call order, in the
 * caller's observation order.
 *   group == NULL: every observation is its own group (classic LOO); ngroups is ignored, G_b = n_b.
 *   group != NULL: group[i] in [-1, ngroups[b]); -1 = never held out (always conditioned on; its mean and var are NaN).  The
 *     patient's meta as group with ngroups[b] = D is leave-one-covariate-out.  An id outside the range: MEDGP_ERR_ARG before
 *     any device work.
 *   mean[i], var[i]: mean and variance of y_i (noise included) given all observations of the patient outside i's group.
 *   lpd: sum_b G_b entries, patient b's at sum_{a<b} G_a, one per group id (observation order for group == NULL): the joint log
 *     density of the group's held-out values; 0.0 for an empty group.  total[b]: the sum of the patient's lpd in group-id order
 *     (the LOO / LGO log pseudo-likelihood).
 *   group_status: laid out as lpd; 0 ok, -1 when the factorisation of M met a pivot <= 0 or NaN (no jitter loop here, as for
 *     cov_status; impossible in exact arithmetic): the group's outputs are NaN then.
 * Any of mean, var, lpd, total, group_status may be NULL, but not all of mean, var, lpd and total.  A patient with
 * status[b] < 0 gets NaN everywhere and group_status -1.
 * log 2 pi uses the context's pi (medgp_set_pi): one group holding all n observations gives lpd = -nlml of medgp_nlml_grad
 * without a prior.  Priors play no part.  After k jitter rounds every quantity is that of the matrix that was factored,
 * K + k diag(sigma^2).  A group's outputs depend only on the patient, theta and the group's members: not on the labels, the
 * other groups, the batch-mates (route pinned) or the launch chunks.  The blocks of a launch chunk (2 m'^2 + 2 m' doubles per
 * group of more than one observation, m' = its size rounded up to 64) stay within MEDGP_POSTERIOR_BUDGET_GB; a single group
 * beyond it fails with MEDGP_ERR_CAPACITY, as does a call whose per-entry matrices exceed the memory budget.  M is factored by
 * one workgroup per group.  medgp_get_factor is valid afterwards (the call forms alpha and L^-1).
 * Supported range of the time stamps: |t| <= 2^14 h (medgp_set_patient).  mean and var keep the bar of 2 fp32 ulps over the whole
 * range.  lpd and total are fp64 outputs of a K formed from the cos / sin (w t_i) tables, and lose |w t| eps like them: within
 * 1e-10 max(1, |ref|) near the origin (tests/test_loo_gpu.py, |t| <= 200 h), but an fp64 program that forms K from such tables is
 * itself off by 8.8e-11 at |t| = 2^14 h and a period of 1 h (1.3e-11 at 12 h, 8.5e-13 at 72 h; tests/golden/time_shift_spread.json),
 * so away from the origin the bound is max(1e-10, 50 x that table error) max(1, |ref|): 4.4e-9 at 2^14 h and 1 h.  The device's worst
 * there was 8.8e-11 (tests/test_time_shift_gpu.py prints it).  All pointers are HOST memory. */
int medgp_loo_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int32_t *group,
                    const int32_t *ngroups, float *mean, float *var, double *lpd, double *total, int32_t *status,
                    int32_t *group_status);

/* The negative leave-one-out log pseudo-likelihood as a training objective, with its gradient in the hyper-parameters: the second
 * model-selection criterion of a GP beside the marginal likelihood (Rasmussen & Williams 5.4.2).  The reference has no such output;
 * the definition is the long-double restatement in tests/loo_grad_truth.py.  With
 *   P = K^-1,  alpha = P y,  d_i = P_ii,  u_i = alpha_i / d_i,  s_i = (1 + alpha_i^2 / d_i) / d_i,  v = P u,
 *   log p(y_i | y_-i) = 1/2 log d_i - 1/2 alpha_i^2 / d_i - 1/2 log 2 pi,
 *   J = - sum_i log p(y_i | y_-i),
 *   dJ / d theta_h = 1/2 tr(W_loo dK / d theta_h),   W_loo = P diag(s) P - (alpha v^T + v alpha^T)       (from R&W eq. 5.13):
 * the marginal-likelihood gradient with W_loo in the place of W = K^-1 - alpha alpha^T.
 * nbatch, slots, theta, status as medgp_loo_batch (one factorisation per patient, no n > 2 guard; status[b] = jitter rounds or -1).
 *   obj[b] = J plus the prior term exactly as medgp_nlml_grad adds it for that slot; without a prior it is -total[b] of
 *     medgp_loo_batch(group = NULL).  log 2 pi uses the context's pi (medgp_set_pi).
 *   grad[b * H ..]: dJ / d theta in theta order, the prior's gradient contribution applied as in medgp_nlml_grad (a clamp prior
 *     zeroes the component).
 *   flag_grad: 0 = the objective only (grad may be NULL; P diag(s) P is never formed), 1 = objective and gradient; any other
 *     bit, or grad == NULL with flag_grad = 1: MEDGP_ERR_ARG before any device work.
 * After k jitter rounds every quantity is that of the matrix that was factored, K + k diag(sigma^2), and the W -> gradient
 * mapping is unchanged: the noise gradient is not scaled by 1 + k (as for medgp_nlml_grad).  A patient with status[b] < 0 gets
 * NaN obj and grad.  All three covariance families; Q <= 16 only: Q > 16 returns MEDGP_ERR_ARG (the generic route of
 * medgp_nlml_grad keeps the full W in the very buffer that holds P here), and MEDGP_V0 is not honoured by this call.  A call
 * whose per-entry matrices exceed the memory budget fails with MEDGP_ERR_CAPACITY, as medgp_loo_batch does.  With the route
 * pinned a patient's obj and grad bits do not depend on its batch-mates or their order: no atomics, every sum in a fixed order.
 * medgp_get_factor is VALID afterwards: the call forms alpha and L^-1 and leaves both untouched (P overwrites the factor L,
 * which medgp_get_factor does not read).
 * Supported range of the time stamps: |t| <= 2^14 h (medgp_set_patient).  obj and grad are held to the fp64 budget of
 * tests/loo_grad_truth.py near the origin; K and the gradient factors come from the cos / sin (w t_i) tables, so at an offset the
 * budget is the larger of that and M x the error of an fp64 table program there (M = 256 objective, 128 gradient): measured table
 * errors at 2^14 h and a period of 1 h 2.0e-12 (objective) and 5.2e-11 (gradient), at 12 h 6.9e-14 and 1.0e-11
 * (tests/golden/time_shift_spread.json); the device's were the same to two digits (tests/test_time_shift_gpu.py).
 * All pointers are HOST memory. */
int medgp_loo_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int flag_grad, double *obj,
                   double *grad, int32_t *status);

/* The negative leave-group-out log pseudo-likelihood as a training objective, with its gradient in the hyper-parameters: what
 * medgp_loo_batch reports for any partition of a patient's observations (a covariate from the other covariates, a time window from
 * the rest of the stay), made optimisable.  medgp_loo_grad is its special case of singleton groups.  The reference has no such
 * output; the definition is the long-double restatement in tests/lgo_grad_truth.py.  K is the matrix that was factored (noise
 * included), P = K^-1, alpha = P y, and B_g the ascending index set of every non-empty group g >= 0:
 *   M_g = P[B_g, B_g],   r_g = M_g^-1 alpha_{B_g},
 *   lpd_g = -1/2 alpha_{B_g}^T r_g + 1/2 log det M_g - |B_g| / 2 log 2 pi                      (exactly medgp_loo_batch's lpd),
 *   J = - sum_g lpd_g,
 *   S = sum_g E_g (M_g^-1 + r_g r_g^T) E_g^T     (block-"diagonal" on the groups' index sets, zero on id -1),
 *   r = sum_g E_g r_g,   v = P r,
 *   dJ / d theta_h = 1/2 tr(W_lgo dK / d theta_h),     W_lgo = P S P - (alpha v^T + v alpha^T):
 * the marginal-likelihood gradient with W_lgo in the place of W = K^-1 - alpha alpha^T.  All groups singletons: W_lgo = W_loo of
 * medgp_loo_grad.  One group holding all n observations: J is the nlml of medgp_nlml_grad without a prior and W_lgo = W.
 * nbatch, slots, theta, status as medgp_loo_grad (no n > 2 guard; status[b] = jitter rounds or -1).
 *   group, ngroups: as medgp_loo_batch -- group[i] in [-1, ngroups[b]), concatenated by patient in call order, in the caller's
 *     observation order; -1 = never held out.  An id outside the range, a negative ngroups[b], or ngroups == NULL with group ids:
 *     MEDGP_ERR_ARG before any device work.  group == NULL is classic LOO: the call is medgp_loo_grad's, bit for bit (ngroups must
 *     be NULL too; G_b = n_b).
 *   obj[b] = J plus the prior term exactly as medgp_nlml_grad adds it for that slot; without a prior it is -total[b] of
 *     medgp_loo_batch with the same groups.  An empty group contributes 0; a patient with no scored observation has J = 0 and the
 *     prior's gradient alone.  log 2 pi uses the context's pi (medgp_set_pi).
 *   grad[b * H ..], flag_grad: as medgp_loo_grad (0 = the objective only: neither P nor S is formed, the same bits of obj; any other
 *     bit, or grad == NULL with flag_grad = 1: MEDGP_ERR_ARG before any device work).
 *   group_status (may be NULL): laid out as medgp_loo_batch's; 0 ok, -1 when the factorisation of M_g met a pivot <= 0 or NaN: that
 *     patient's obj and grad are NaN then, other patients are untouched.  A patient with status[b] < 0 gets NaN obj and grad and
 *     group_status -1.
 * After k jitter rounds every quantity is that of the matrix that was factored, K + k diag(sigma^2), and the noise gradient is not
 * scaled by 1 + k.  All three covariance families; Q <= 16 only: Q > 16 returns MEDGP_ERR_ARG, and MEDGP_V0 is not honoured by this
 * call.  A call whose per-entry matrices exceed the memory budget fails with MEDGP_ERR_CAPACITY (no memory waves), as does a single
 * group whose block (2 m'^2 + 2 m' doubles, m' = its size rounded up to 64) exceeds MEDGP_POSTERIOR_BUDGET_GB; the blocks of a launch
 * chunk stay within that budget, and a gradient call holds one more ldn^2 matrix per entry (P S) in a buffer of its own.
 * No atomics, every sum in a fixed order over the patient's own operands: with the route pinned a patient's obj and grad bits do not
 * depend on its batch-mates, their order, the labels of its groups or the launch chunks.  medgp_get_factor is VALID afterwards (P
 * overwrites the factor L, which it does not read; L^-1, alpha and the log determinant are left untouched).
 * Supported range of the time stamps: |t| <= 2^14 h (medgp_set_patient).  obj and grad are held to the fp64 budget of
 * tests/lgo_grad_truth.py near the origin (|t| <= 200 h); K and the gradient factors come from the cos / sin (w t_i) tables and lose
 * |w t| eps with them away from it, as medgp_loo_grad's.
 * All pointers are HOST memory. */
int medgp_lgo_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int32_t *group,
                   const int32_t *ngroups, int flag_grad, double *obj, double *grad, int32_t *status, int32_t *group_status);

/* Products of the Fisher information of the Gaussian marginal likelihood with vectors: the curvature the four training objectives
 * lack.  With K the matrix that was factored (noise included), P = K^-1 and dK/dtheta_h the derivative of the UN-jittered K the
 * gradient calls use,
 *   F_hk(theta) = 1/2 tr(P dK/dtheta_h P dK/dtheta_k),
 *   (F v)_h = 1/2 tr(W_F dK/dtheta_h),     W_F = P Kdot P,     Kdot = sum_k v_k dK/dtheta_k:
 * the marginal-likelihood gradient with W_F in the place of W.  F is the expected Hessian of the nlml: positive semi-definite,
 * independent of y, first derivatives of the kernel only.  The reference has no such output; the definition is the long-double
 * restatement in tests/fisher_truth.py (dgram_dir is Kdot, fisher_vec the product).  With it a host can run Fisher scoring or
 * natural-gradient CG, form a patient's full F for small H, and report Cramer-Rao standard errors (medgp_amd.information).
 * nbatch, slots, theta, status as medgp_loo_grad (one factorisation per patient, no n > 2 guard; status[b] = jitter rounds or -1).
 *   nvec >= 1 directions per entry; vec[(b * nvec + j) * H ..] is direction j of entry b in theta order (v lives in theta space: a
 *     patient not uploaded grouped by output gives the result of the grouped upload); fvec has the same layout and holds F(theta_b) v_bj.
 *     nvec < 1, or NULL vec, fvec, theta or slots: MEDGP_ERR_ARG before any device work.
 * After k jitter rounds P is the inverse of K + k diag(sigma^2); the noise hyper log sigma_d still contributes 2 sigma_d^2 on the
 * diagonal entries of covariate d to Kdot, not scaled by 1 + k.  Priors play no part: F is the information of the likelihood, and a
 * slot's prior descriptor does not change a bit of the output; neither does y.  A patient with status[b] < 0 gets NaN in all its
 * nvec * H outputs, its batch-mates are untouched.
 * All three covariance families; Q <= 16 only: Q > 16 returns MEDGP_ERR_ARG, and MEDGP_V0 is not honoured by this call.  The call
 * holds two more ldn^2 matrices per entry (Kdot and T = P Kdot) in buffers of its own, reused by every direction; a call whose
 * per-entry matrices -- all four -- exceed the memory budget fails with MEDGP_ERR_CAPACITY (no memory waves).
 * No atomics, every sum in a fixed order over the entry's own operands: with the route pinned a direction's fvec bits depend on the
 * patient, theta and that direction alone -- not on the batch-mates, on nvec, on the direction's position j or on the other
 * directions.  medgp_get_factor is VALID afterwards (P overwrites the factor L, which it does not read; L^-1, alpha and the log
 * determinant are left untouched).
 * Out of scope: curvature of the priors; curvature of the cross-validation objectives; Q > 16.  (The exact Hessian: medgp_hess_vec.)
 * All pointers are HOST memory. */
int medgp_fisher_vec(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int nvec, const double *vec, double *fvec,
                     int32_t *status);

/* Products of the exact (observed) Hessian of the data term of the negative log marginal likelihood with vectors.  With
 *   L(theta) = 1/2 y^T K^-1 y + 1/2 log det K + const     (medgp_nlml_grad's objective without the prior stage),
 * K the matrix that was factored, P = K^-1, alpha = P y, W = P - alpha alpha^T (grad L_h = 1/2 tr(W dK/dtheta_h)) and
 *   Kdot = sum_k v_k dK/dtheta_k,     beta = P Kdot alpha,     Wdot = -P Kdot P + beta alpha^T + alpha beta^T,
 *   (grad^2 L v)_h = 1/2 tr(Wdot dK/dtheta_h) + 1/2 tr(W dKdot/dtheta_h):
 * the first term is the gradient with Wdot in the place of W, the second needs the second derivatives of the kernel, which come from
 * five block sums of W per mixture component formed once per call (two more than the gradient's).  Unlike the Fisher information the
 * result depends on y and need not be positive semi-definite.  The reference has no such output; the definition is the long-double
 * restatement in tests/hess_truth.py (hess_vec).  With it a host can take Newton-CG / trust-region steps, check that a trained theta
 * is a minimum, and form a Laplace approximation of the hyper posterior (medgp_amd.curvature).
 * nbatch, slots, theta, nvec, vec, status and the layout of hvec are exactly those of medgp_fisher_vec (one factorisation per patient,
 * no n > 2 guard; status[b] = jitter rounds or -1; NULL slots, theta, vec or hvec, or nvec < 1: MEDGP_ERR_ARG before any device work).
 *   grad: NULL, or [nbatch * H]: the gradient of L (no prior term), from the block sums the call forms anyway.
 * Jitter convention, as medgp_fisher_vec: after k jitter rounds P and alpha belong to K + k diag(sigma^2); every kernel derivative,
 * first and second, is that of the UN-jittered K and is not scaled by 1 + k (so the result is the Hessian of L at zero rounds only).
 * Priors play no part: a slot's prior descriptor does not change a bit of any output.  A patient with status[b] < 0 gets NaN in all
 * its nvec * H outputs (and its H gradient entries), its batch-mates are untouched.
 * All three covariance families; Q <= 16 only: Q > 16 returns MEDGP_ERR_ARG, and MEDGP_V0 is not honoured by this call.  Memory as
 * medgp_fisher_vec: Kdot and T = P Kdot in buffers of the call, MEDGP_ERR_CAPACITY when the four per-entry matrices exceed the memory
 * budget (no memory waves).  No atomics, every sum in a fixed order over the entry's own operands: with the route pinned a direction's
 * bits depend on the patient, theta and that direction alone.  medgp_get_factor is VALID afterwards, as after medgp_fisher_vec.
 * Out of scope: curvature of the priors (medgp_amd.curvature.prior_curvature adds it on the host), of the cross-validation and
 * forecast objectives; Q > 16.
 * All pointers are HOST memory. */
int medgp_hess_vec(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int nvec, const double *vec, double *hvec,
                   double *grad, int32_t *status);

/* Hyper-sensitivity of predictions: the directional derivatives (JVP) of the posterior mean and variance at every test point along
 * directions in theta space, all from ONE factorisation per patient.  With K the matrix that was factored, P = K^-1, alpha = P y,
 * Kdot = sum_k v_k dK/dtheta_k of the UN-jittered K with its noise diagonal 2 sigma_d^2 v_sigma,d (medgp_fisher_vec's Kdot) and, for
 * test point j with covariate m_j and time t*_j,
 *   k_j       the column of K* (medgp_posterior_batch),     w_j = P k_j,     u = Kdot alpha,
 *   kdot_j    = sum_q e ((Bdot_q[m_i,m_j] + cv_q dt^2 B_q[m_i,m_j]) cos(w_q dt) + cmu_q dt B_q[m_i,m_j] sin(w_q dt)),   dt = t_i - t*_j,
 *               e = exp(-c_q dt^2): the Kdot element with the same coefficient block Bdot, cmu, cv, without a noise term,
 *   kdot**_j  = sum_q Bdot_q[m_j,m_j],     sigdot_j = 2 sigma^2_{m_j} v_sigma,m_j:
 *   mean_j = k_j^T alpha                        dmean_j = kdot_j^T alpha - w_j^T u
 *   var_j  = k**_j - k_j^T P k_j + sigma^2      dvar_j  = kdot**_j + sigdot_j - 2 kdot_j^T w_j + w_j^T Kdot w_j
 * dvar is the derivative of the unclamped predictive variance, noise included once, as var is.  The reference has no such output;
 * the definition is the long-double restatement in tests/posterior_jvp_truth.py (jvp).  With it a host forms the delta-method
 * (Laplace) predictive variance var + sum_r (dmean . s_r)^2 for a factor S S^T of the hyper covariance, and the sensitivity of a
 * prediction to each hyper group (medgp_amd.sensitivity).
 * nbatch, slots, theta, offsets, meta2, t2 and status mean exactly what they mean for medgp_posterior_batch: one factorisation per
 * patient, no n > 2 guard, status[b] = jitter rounds or -1, an empty range of points is allowed, meta2 may be NULL for SE / SM.
 *   nvec >= 1 directions per entry; vec[(b * nvec + k) * H ..] is direction k of entry b in theta order, exactly as medgp_fisher_vec.
 *   dmean[j * nvec + k], dvar[j * nvec + k]   fp64, required; j counts the points of the call (offsets[b] + i).
 *   mean[j], var[j]   may both be NULL.  When given: the plug-in posterior, held to medgp_posterior_batch's own bar (2 fp32 ulps of
 *     tests/posterior_ref.py).  Bit identity with that call is NOT promised: this call holds the inverse factor, that one does not.
 *   nvec < 1, or NULL slots, theta, offsets, vec, dmean or dvar, or only one of mean / var: MEDGP_ERR_ARG before any device work.
 * Jitter convention, as medgp_fisher_vec: after k jitter rounds P and alpha belong to K + k diag(sigma^2); Kdot, kdot_j, kdot**_j and
 * sigdot_j are those of the UN-jittered kernel and are not scaled by 1 + k, so the result is a true derivative at zero rounds only.
 * A patient with status[b] < 0 gets NaN in all its outputs (mean, var and the nvec derivatives of each of its points); its
 * batch-mates are untouched.
 * All three covariance families; Q <= 16 only: Q > 16 returns MEDGP_ERR_ARG, and MEDGP_V0 is not honoured by this call.  Memory: one
 * more ldn^2 matrix per entry (Kdot) in a buffer of the call, reused by every direction, and two ldn x 64 panels of work rows per tile
 * of 64 points (W = P K* and V = L^-1 K*).  The points are cut into launches whose work rows stay within MEDGP_POSTERIOR_BUDGET_GB, as
 * medgp_posterior_batch's are; a call whose per-entry matrices -- all three -- exceed the memory budget fails with
 * MEDGP_ERR_CAPACITY (no memory waves).  Supported range of the time stamps: |t| <= 2^14 h, as the posterior call (K*, Kdot and kdot
 * come from cos / sin tables of the observations and of the test points and lose |w t| eps away from the origin).
 * Determinism: no atomics, every sum in a fixed order over the entry's own operands.  With the route pinned the bits of
 * (point j, direction k) depend on the patient, theta, that point and that direction alone -- not on the batch-mates, on nvec, on the
 * direction's position, on the other points or their order, on the tile a point lands in, or on how the call is cut into launches.
 * medgp_get_factor is VALID afterwards: the call overwrites neither L nor L^-1, alpha or the log determinant.
 * Out of scope: Q > 16; derivatives of parts, of the joint covariance, of trend, components and functionals; the second-order mean
 * correction.  The reverse mode is medgp_posterior_vjp_batch.
 * All pointers are HOST memory. */
int medgp_posterior_jvp_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                              const int32_t *meta2, const float *t2, int nvec, const double *vec, float *mean, float *var, double *dmean,
                              double *dvar, int32_t *status);

/* The reverse mode of medgp_posterior_jvp_batch: the gradient over ALL hypers of any scalar loss of the predictions, from ONE
 * factorisation per patient and one weighted gradient pass (about the work of one medgp_nlml_grad plus the W = K^-1 K* solve the JVP
 * call has), instead of one JVP direction per hyper.  For cotangents cm_j = dloss/dmean_j, cv_j = dloss/dvar_j at the test points,
 *   grad_h = sum_j cm_j dmean_j/dtheta_h + cv_j dvar_j/dtheta_h,
 * with mean, var, dmean and dvar exactly those of medgp_posterior_jvp_batch.  The definition is the identity with the JVP: for every
 * direction v, grad . v = sum_j cm_j dmean_j(v) + cv_j dvar_j(v); its long-double restatement is tests/posterior_vjp_truth.py.  With
 * c = W cm and Wc = W diag(cv) the device evaluates  1/2 tr(G dK/dtheta_h),  G = 2 Wc W^T - (c alpha^T + alpha c^T)  (the nlml gradient's
 * reduction with G in the place of K^-1 - alpha alpha^T; G never reaches memory),  sum_ij R_ij dk*_ij/dtheta_h,  R = alpha cm^T - 2 Wc,
 * and the test-diagonal terms  sum_j cv_j (sum_q dB_q[m_j,m_j]/dtheta_h + 2 sigma^2_{m_j} [h = sigma_{m_j}]).
 * nbatch, slots, theta, offsets, meta2, t2, mean, var and status mean exactly what they mean for medgp_posterior_jvp_batch: one
 * factorisation per patient, no n > 2 guard, status[b] = jitter rounds or -1, an empty range of points is allowed (its gradient is
 * zero, its built-in loss 0), meta2 may be NULL for SE / SM, mean / var are both given or both NULL and held to tests/posterior_ref.py's
 * 2-ulp bar.
 *   loss_kind = MEDGP_PLOSS_CUSTOM (0): cot_mean[j * ncot + k], cot_var[j * ncot + k] are the caller's cotangents of point j (counting
 *     the points of the call) in set k, ncot >= 1; grad[(b * ncot + k) * H ..] is the gradient of set k over the points of entry b.
 *     loss, y2 and wt must be NULL.  ncot > 1 serves Jacobian rows of a few points: cheaper than H JVP directions when m < H.
 *   Built-in kinds: the device forms the cotangents in fp64 from its own fp64 mean_j, var_j (the float outputs are roundings of
 *     the same quantities, not their source), so a held-out score and its gradient cost one factorisation.  ncot must be 1, cot_mean
 *     and cot_var NULL, y2[j] and loss are required, wt[j] is optional (NULL = 1; it multiplies l_j).  loss[b] = sum_j wt_j l_j, summed
 *     in the caller's point order; grad[b * H ..] its gradient.
 *       MEDGP_PLOSS_NLPD (1)   l = 1/2 log(2 pi var) + (y - mean)^2 / (2 var), with the true pi (medgp_set_pi plays no part)
 *       MEDGP_PLOSS_SQERR (2)  l = (y - mean)^2
 *       MEDGP_PLOSS_CRPS (3)   s = sqrt(var), z = (y - mean) / s:  l = s (z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi));
 *                              dl/dmean = -(2 Phi(z) - 1),  dl/dvar = (2 phi(z) - 1 / sqrt(pi)) / (2 s)
 *     var is the unclamped predictive variance with the noise included once, as in the JVP call.  A non-positive (or NaN) var_j
 *     under NLPD / CRPS makes that entry's loss and every line of its grad NaN; its batch-mates are untouched.
 *   An unknown kind, ncot < 1, ncot != 1 with a built-in kind, missing or superfluous cot_mean / cot_var / y2 / loss / wt, only one
 *     of mean / var, NULL slots, theta, offsets or grad: MEDGP_ERR_ARG before any device work.
 * Conventions of the JVP call, unchanged.  Jitter: after k rounds P and alpha belong to K + k diag(sigma^2) while the derivatives are
 * those of the UN-jittered kernel and are not scaled by 1 + k.  Priors play no part: a prior descriptor changes no bit.  A patient with
 * status[b] < 0 gets NaN in loss, grad, mean and var; its batch-mates are untouched.  All three covariance families; Q <= 16 only
 * (Q > 16: MEDGP_ERR_ARG; 8 < Q <= 16 runs the tile kernel twice), MEDGP_V0 is not honoured.  |t| <= 2^14 h.  medgp_get_factor is VALID
 * afterwards with the bits it has after medgp_nlml_grad: the call overwrites neither L nor L^-1, alpha or the log determinant.
 * Memory: no matrix beyond the two of the factorisation; two ldn x 64 panels of work rows per tile of 64 points.  The work rows of all
 * tiles of an entry are resident for its product, so the call is cut into launches BETWEEN entries, within MEDGP_POSTERIOR_BUDGET_GB;
 * one entry alone beyond that budget, or per-entry matrices beyond the memory budget: MEDGP_ERR_CAPACITY (no memory waves).
 * Determinism: no atomics, every sum in a fixed order over the entry's own operands.  The host sorts every patient's points by
 * covariate (stable) before the upload.  With the route pinned the bits of (entry, set) depend on the patient, theta, its points and
 * that set alone -- not on the batch-mates, on ncot or the set's position, on whether mean / var are asked for, or on how the call is
 * cut into launches.  They DO depend on the order of the points that share a covariate (independence of the points' order is NOT
 * promised); a built-in kind and the custom kind fed the same cotangents agree to rounding of the cotangents, not to bits.
 * Out of scope: Q > 16; cotangents of parts, joint covariance, trend, components and functionals; the Hessian of a predictive loss;
 * priors (add medgp_nlml_grad's prior lines on the host if wanted); device-resident theta / cotangents.
 * All pointers are HOST memory. */
#define MEDGP_PLOSS_CUSTOM 0
#define MEDGP_PLOSS_NLPD   1
#define MEDGP_PLOSS_SQERR  2
#define MEDGP_PLOSS_CRPS   3
int medgp_posterior_vjp_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                              const int32_t *meta2, const float *t2, int loss_kind, const double *y2, const double *wt, int ncot,
                              const double *cot_mean, const double *cot_var, float *mean, float *var, double *loss, double *grad,
                              int32_t *status);
/* The fp64 plug-in mean and var the LAST medgp_posterior_vjp_batch of this context evaluated on the device -- the quantities its
 * built-in kinds form their cotangents from; the float mean / var of that call are held to the posterior call's bar, these to the
 * fp64 budget -- in the caller's point order (M = offsets[nbatch] of that call, else MEDGP_ERR_ARG; NaN for a patient with
 * status < 0).  A caller that forms its own cotangents in fp64 (medgp_amd.predictive.TorchPosterior) reads them here.  Valid until
 * the next medgp_posterior_vjp_batch of the context; without one before it: MEDGP_ERR_ARG.  Host pointers. */
int medgp_posterior_vjp_moments(medgp_ctx *ctx, int64_t M, double *mean, double *var);

/* A constant BASELINE per covariate, fixed or integrated out (ABI 20).  Every other call has a zero mean: between observations and at
 * every forecast horizon a patient's covariates revert to 0, the cohort mean after z-scoring.  Here y = H beta + f + noise with
 * H[i, d] = [m_i = d] (n x D; SE / SM: D = 1) and
 *   mode = MEDGP_MEAN_FIXED (1)     beta = b0: the reference's c_meanfunc_constMO with b0 its mean hypers (the scalar c_meanfunc_const is
 *                                   the D = 1 case); lam is ignored and may be NULL
 *        ref: mean/c_meanfunc_constMO.cpp (compute_mean_vector / compute_mean_gradients), inference/c_inference_exact.cpp:77-80, 221-232
 *   mode = MEDGP_MEAN_MARGINAL (0)  beta_d ~ N(b0_d, 1 / lam_d) integrated out in closed form (Rasmussen & Williams section 2.7): no
 *                                   further hyper to optimise.  lam_d = 0 is the flat prior (eq. 2.45); (0, 1) suits z-scored data.
 * theta keeps the context's H hypers (medgp_num_hyp): the mean is a separate argument.  b0 and lam are [nbatch][D], row b for patient b.
 * With K the matrix the pipeline factored (after its jitter rounds, as everywhere), P = K^-1, G = L^-1 H, Lambda = diag(lam),
 * r0 = y - H b0 (the definition is tests/mean_truth.py, in long double):
 *   A = Lambda + G^T G,  c = G^T L^-1 r0,  beta^ = b0 + A^-1 c,  alpha~ = P (y - H beta^),  W~ = P - P H A^-1 H^T P - alpha~ alpha~^T
 *   nlml[b]  = 1/2 (r0^T P r0 - c^T A^-1 c) + 1/2 log|K| + 1/2 log|A| - 1/2 sum_{lam_d > 0} log lam_d + 1/2 (n - #{lam_d = 0}) log 2 pi
 *              (all lam_d > 0: exactly -log N(y; H b0, K + H Lambda^-1 H^T)), minus the log prior of theta as medgp_nlml_grad
 *   grad[b]  = 1/2 tr(W~ dK/dtheta_h), the prior lines as medgp_nlml_grad; the noise lines from diag(W~), not scaled by jitter rounds
 *   dmean[b] = d nlml / d b0_d = -lam_d (beta^_d - b0_d) = -(H^T alpha~)_d
 *   beta[b] = beta^,  beta_cov[b] = A^-1 ([D][D], symmetric): d nlml / d lam_d = 1/2 (A^-1)_dd + 1/2 (beta^_d - b0_d)^2 - 1/(2 lam_d)
 *              is formed from them on the host (medgp_amd.baseline.prior_grad)
 * FIXED: alpha~ = P r0, W~ = P - alpha~ alpha~^T, nlml = 1/2 r0^T alpha~ + 1/2 log|K| + 1/2 n log 2 pi, dmean_d = -sum_{m_i = d} alpha~_i,
 * beta = b0, beta_cov = 0.  With b0 = 0 it is medgp_nlml_grad to rounding (another summation order: not to bits).
 * The quadratic form is evaluated as |L^-1 r0 - G (beta^ - b0)|^2 + sum_d lam_d (beta^_d - b0_d)^2, a sum of squares: nothing cancels
 * where lam is small.
 * A covariate WITHOUT observations has a zero column in H: with lam_d > 0, beta^_d = b0_d and the predictive variance gains 1 / lam_d;
 * with lam_d = 0 (MARGINAL) the model is improper for that entry: status -1, decided on the device; batch-mates are unaffected.
 * status[b]: jitter rounds, or -1 (n <= 2 as medgp_nlml_grad, a failed factorisation, an improper entry, a failed pivot of A); the
 * entry's outputs are then NaN.  flag_grad = 0: nlml, dmean, beta and beta_cov alone.  Every output pointer may be NULL.
 * MEDGP_ERR_ARG before any device work: mode outside the two values, lam NULL in MARGINAL mode, a negative or NaN lam, a non-finite b0,
 * Q > 16.  MEDGP_ERR_CAPACITY: D > 64 (the rank-D correction is ONE 64-column panel and A lives in LDS), and a call whose two
 * per-entry matrices and three n x 64 panels exceed the memory budget (no memory waves, as medgp_fisher_vec).
 * Blocking.  Route selection, size classes and medgp_pin_route as medgp_nlml_grad; the generic kernels (MEDGP_V0) are not honoured.
 * No atomics: with the route pinned an entry's bits depend on the patient, theta, b0, lam and mode alone -- not on batch-mates,
 * position, batch size or how the call is cut into launches.
 * Accuracy: tests/test_mean_gpu.py holds every output to the fp64 budget M_MEAN max(E_programs, 2^-53) of tests/mean_truth.py.
 * All pointers are HOST memory. */
#define MEDGP_MEAN_MARGINAL 0
#define MEDGP_MEAN_FIXED    1
int medgp_mean_nlml_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int mode,
                         const double *b0 /* [nbatch][D] */, const double *lam /* [nbatch][D]; NULL in FIXED mode */, int flag_grad,
                         double *nlml, double *grad /* [nbatch][H] */, double *dmean /* [nbatch][D] */, double *beta /* [nbatch][D] */,
                         double *beta_cov /* [nbatch][D][D] */, int32_t *status);
/* The posterior at test points (m*_j, t*_j) under the same model, from ONE factorisation per patient.  With V_j = L^-1 k*_j and
 * r_j = e_{m*_j} - G^T V_j:
 *   mean[j] = V_j^T z + r_j^T beta^                                        (the zero-mean posterior mean plus the baseline's share)
 *   var[j]  = (k** - V_j^T V_j + sigma^2_{m*_j}) + r_j^T A^-1 r_j          (FIXED: the last term is absent)
 * fp64 outputs in the caller's point order; offsets / meta2 / t2 as medgp_posterior_batch (meta2 may be NULL for SE / SM and is
 * range-checked for LMC-SM; a patient without points is allowed); no n > 2 guard, as there.  mode, b0, lam, beta, the improper-entry
 * rule, the argument errors and the capacity rules as medgp_mean_nlml_grad; the work rows are chunked within
 * MEDGP_POSTERIOR_BUDGET_GB.  The points of a patient with status[b] < 0 get NaN.  mean and var: both or neither may be NULL.
 * A point's bits depend on the patient, theta, b0, lam, mode and that point alone: not on the other points or their ORDER, the tile or
 * column it lands in, the launch chunk, or -- with the route pinned -- the batch-mates.
 * Supported range of the time stamps: |t| <= 2^14 h, as medgp_posterior_batch.  All pointers are HOST memory. */
int medgp_mean_posterior_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0,
                               const double *lam, const int64_t *offsets, const int32_t *meta2, const float *t2,
                               double *mean, double *var /* fp64, [M] */, double *beta /* [nbatch][D] */, int32_t *status);

/* FIXED EFFECTS with a general basis (ABI 21): the baseline calls' model y = H beta + f + noise with ANY H (n x p) in place of the
 * indicator H[i, d] = [m_i = d] -- a linear drift per covariate, a step or ramp that is 1 while a drug runs (its coefficient, with its
 * posterior standard deviation, says whether and by how much the intervention moved the covariate), a time-of-day harmonic shared by
 * several covariates, a dose-proportional column (medgp_amd.basis builds them for observations and test points alike).
 *
 * medgp_set_basis -- a resident basis per slot: hmat holds rows [offsets[k], offsets[k+1]) x p (row-major, fp64) for slots[k], in the
 * CALLER's observation order of the patient currently uploaded there (rows must equal its n).  hmat == NULL removes the basis of the
 * listed slots (p and offsets are then ignored).  The basis is uploaded once, like medgp_set_patients and medgp_set_priors: H does not
 * change between the evaluations of a training loop.  The library brings the rows into its grouped order, packs all listed slots into
 * one pinned buffer and sends them in ONE host-to-device transfer; nothing waits for the device.  All device memory of the bases is
 * obtained here, never inside an evaluation call: a call that repeats an earlier one (same slots, same order, same sizes) overwrites
 * its rows in place, any other is placed behind what is in use, and when that does not fit the live bases are compacted into a
 * larger block.  A later medgp_set_patient[s] on a slot DROPS that slot's basis (the rows no longer belong to the data); an evaluation
 * on a slot without a basis returns MEDGP_ERR_ARG before any device work, as does a call whose slots do not all carry the same p.
 * 1 <= p <= 64: p < 1 is MEDGP_ERR_ARG, p > 64 MEDGP_ERR_CAPACITY (one 64-column panel, A in LDS, as D <= 64 of the baseline calls).
 * MEDGP_ERR_ARG: a non-finite entry, a row count different from the slot's n, a slot without a patient, a slot listed twice. */
int medgp_set_basis(medgp_ctx *ctx, int nslots, const int32_t *slots, int p, const int64_t *offsets, const double *hmat);
/* medgp_mean_nlml_grad with H from the resident basis and p in place of D; mode takes MEDGP_MEAN_MARGINAL / MEDGP_MEAN_FIXED.  b0 and
 * lam are [nbatch][p].  With K the matrix the pipeline factored, P = K^-1, G = L^-1 H, Lambda = diag(lam), r0 = y - H b0, w = L^-1 r0
 * (the definition is tests/basis_truth.py, in long double):
 *   A = Lambda + G^T G,  c = G^T w,  delta = A^-1 c,  beta^ = b0 + delta,  alpha~ = P (y - H beta^),  W~ = P - P H A^-1 H^T P - alpha~ alpha~^T
 *   nlml[b]  = 1/2 quad + 1/2 log|K| + 1/2 log|A| - 1/2 sum_{lam_c > 0} log lam_c + 1/2 (n - #{lam_c = 0}) log 2 pi, minus the log prior
 *              of theta as medgp_nlml_grad; quad = r0^T P r0 - c^T A^-1 c evaluated as |w - G delta|^2 + sum_c lam_c delta_c^2
 *   grad[b]  = 1/2 tr(W~ dK/dtheta_h), the prior lines as medgp_nlml_grad; the noise lines from diag(W~), not scaled by jitter rounds
 *   dbeta[b] = d nlml / d b0 = -lam o delta (MARGINAL), -G^T w = -H^T alpha~ (FIXED)
 *   beta[b] = beta^,  beta_cov[b] = A^-1 ([p][p], symmetric; FIXED: beta = b0, beta_cov = 0)
 * There is no segment table to consult for an improper entry: under lam_c = 0 a basis whose flat-prior columns are linearly dependent
 * on the patient's rows makes A singular, and the failed pivot of its factorisation gives status -1 on the device; batch-mates are
 * unaffected.  A pivot fails when it is NaN or not above 4 p 2^-52 times the column's own diagonal entry of A: rounding leaves noise
 * of either sign where an exactly dependent column's pivot would be 0, so "pivot <= 0" alone would pass half of such entries.  A zero column with lam_c > 0 is legal: beta^_c = b0_c, and the variance at a point gains h*_c^2 / lam_c.  A NEARLY
 * dependent basis is the caller's to avoid (centre and scale the time of a trend; no column that others almost reproduce):
 * medgp_amd.basis.conditioning measures it.
 * status, the NaN rows of failed entries, flag_grad, "every output pointer may be NULL", the argument errors (mode, lam, b0, Q > 16),
 * the capacity rule of the per-entry matrices and panels (no memory waves), MEDGP_V0 not honoured, and the determinism promise -- no
 * atomics; with the route pinned an entry's bits depend on the patient, its basis, theta, b0, lam and mode alone, not on batch-mates,
 * position, batch size or launch chunk -- as medgp_mean_nlml_grad.
 * Accuracy: tests/test_basis_gpu.py holds every output to the fp64 budget M_BASIS max(E_programs, 2^-53) of tests/basis_truth.py.
 * All pointers are HOST memory. */
int medgp_basis_nlml_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int mode,
                          const double *b0 /* [nbatch][p] */, const double *lam /* [nbatch][p]; NULL in FIXED mode */, int flag_grad,
                          double *nlml, double *grad /* [nbatch][H] */, double *dbeta /* [nbatch][p] = d nlml / d b0 */,
                          double *beta /* [nbatch][p] */, double *beta_cov /* [nbatch][p][p] */, int32_t *status);
/* medgp_mean_posterior_batch under the same model: h2 holds the basis row h*_j of every test point ([M][p], the caller's point
 * order; required when M > 0, a non-finite entry is MEDGP_ERR_ARG).  With V_j = L^-1 k*_j and r_j = h*_j - G^T V_j:
 *   mean[j] = V_j^T z + r_j^T beta^
 *   var[j]  = (k** - V_j^T V_j + sigma^2_{m*_j}) + r_j^T A^-1 r_j          (FIXED: the last term is absent)
 * Everything else -- offsets / meta2 / t2, the fp64 outputs, a patient without points, NaN for the points of a failed entry, mean and
 * var both or neither, the chunking, the supported range of the time stamps, a point's bits independent of the other points and
 * their order -- as medgp_mean_posterior_batch.  All pointers are HOST memory. */
int medgp_basis_posterior_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int mode, const double *b0,
                                const double *lam, const int64_t *offsets, const int32_t *meta2, const float *t2,
                                const double *h2 /* [M][p]: the basis rows of the test points */,
                                double *mean, double *var /* fp64, [M] */, double *beta /* [nbatch][p] */, int32_t *status);

/* A learned OUTPUT WARP per covariate (ABI 22).  Every other call is Gaussian in the observed value: a lab value is f + noise with
 * symmetric error.  Covariates that are bounded below with a long right tail (INR, creatinine, lactate, bilirubin, white count) are not,
 * also after z-scoring.  A warped GP (Snelson, Rasmussen & Ghahramani 2004) sends the observations through a monotone map g_d per
 * covariate into a space where the GP is Gaussian, and learns the map's parameters together with theta from the exact marginal
 * likelihood.  The family is the sinh-arcsinh transform (Jones & Pewsey 2009): three parameters psi_d = (a_d, eps_d, lambda_d), the
 * identity at psi = 0, skew (eps) and tail weight (lambda) separately, and a closed-form inverse -- so quantiles are exact.
 * For observation i of covariate d = m_i, with delta_d = exp(lambda_d), s_i = asinh(y_i), u_i = delta_d s_i - eps_d:
 *   z_i = g_d(y_i) = a_d + sinh(u_i),   log g'_i = lambda_d + log cosh(u_i) - 1/2 log(1 + y_i^2),
 *   g_d^-1(z) = sinh((asinh(z - a_d) + eps_d) / delta_d)
 * kind[d] = MEDGP_WARP_NONE (0): covariate d is not warped -- z = y exactly, log g' = 0, its three psi entries are ignored and its
 * three dpsi entries are 0.  MEDGP_WARP_SAS (1): the map above.  kind == NULL: all SAS.  kind is [D], shared by the call's patients;
 * psi is [nbatch][D][3], row b for patient b (SE / SM: D = 1).  theta keeps the context's H hypers (medgp_num_hyp).
 * With K the matrix the pipeline factored (after its jitter rounds, as everywhere), P = K^-1, w = L^-1 z, alpha~ = P z (the definition
 * is tests/warp_truth.py, in long double):
 *   nlml[b]   = 1/2 |w|^2 + 1/2 log|K| + 1/2 n log 2 pi - sum_i log g'_i, minus the log prior of theta as medgp_nlml_grad
 *   grad[b]   = 1/2 tr((P - alpha~ alpha~^T) dK/dtheta_h), the prior lines and the noise lines as medgp_nlml_grad
 *   dpsi[b][d][k] = d nlml / d psi_dk = sum_{m_i = d} (alpha~_i dz_i/dpsi_k - dlog g'_i/dpsi_k), with
 *               dz_i/d(a, eps, lambda) = (1, -cosh u_i, delta_d s_i cosh u_i),  dlog g'_i/d(a, eps, lambda) = (0, -tanh u_i, 1 + delta_d s_i tanh u_i);
 *               a covariate without observations: 0 exactly
 *   logjac[b] = sum_i log g'_i
 * At psi = 0, or with every kind NONE, it is medgp_nlml_grad to rounding (another summation order: not to bits).
 * status[b]: jitter rounds, or -1 (n <= 2 as medgp_nlml_grad, a failed factorisation, or a warped observation that is not finite --
 * sinh overflowed; decided on the device, batch-mates are unaffected); the entry's outputs are then NaN.
 * flag_grad = 0: nlml, logjac and dpsi alone (dpsi needs alpha~ but no gradient pass), the same bits as with flag_grad = 1.  Every
 * output pointer may be NULL.
 * MEDGP_ERR_ARG before any device work: a non-finite psi entry, a kind outside {0, 1}, Q > 16.  MEDGP_ERR_CAPACITY: a call whose two
 * per-entry matrices and four vectors exceed the memory budget (no memory waves, as the baseline calls).
 * Blocking.  Route selection, size classes and medgp_pin_route as medgp_nlml_grad; the generic kernels (MEDGP_V0) are not honoured.
 * No atomics: with the route pinned an entry's bits depend on the patient, theta, psi and kind alone -- not on batch-mates, position,
 * batch size or how the call is cut into launches.
 * Accuracy: tests/test_warp_gpu.py holds every output to the fp64 budget M_WARP max(E_programs, 2^-53) of tests/warp_truth.py.
 * NOT provided (out of scope of these two calls): the warp under the LOO, LGO and forecast objectives and in the JVP, VJP, Fisher and
 * Hessian calls; a warp combined with a baseline or a basis in one call; options of medgp_train / medgp_test; other warp families
 * (sums of tanh, Box-Cox); gradients of the predictions in psi.
 * All pointers are HOST memory. */
#define MEDGP_WARP_NONE 0
#define MEDGP_WARP_SAS  1
int medgp_warp_nlml_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int32_t *kind /* [D] or NULL */,
                         const double *psi /* [nbatch][D][3] */, int flag_grad, double *nlml, double *grad /* [nbatch][H] */,
                         double *dpsi /* [nbatch][D][3] */, double *logjac /* [nbatch] */, int32_t *status);
/* The warped posterior at test points (m*_j, t*_j), from ONE factorisation per patient.  With V_j = L^-1 k*_j:
 *   zmean[j] = V_j^T w,   zvar[j] = k** - V_j^T V_j + sigma^2_{m*_j}       (the posterior call's values with w in place of L^-1 y)
 *   quant[j][k] = g^-1_{m*_j}(zmean[j] + zq[k] sqrt(zvar[j]))              zq: nq standard-normal deviates (0: the median); exact
 *                 quantiles of the predictive distribution of the observed value, monotone in zq
 *   lpd[j] = -1/2 log(2 pi zvar[j]) - (g(y2[j]) - zmean[j])^2 / (2 zvar[j]) + log g'(y2[j])      when y2 is given
 * The mean and variance of the observed value have no closed form; they are formed on the host from zmean and zvar by a Gauss-Hermite
 * rule (medgp_amd.warp.moments).  fp64 outputs in the caller's point order; offsets / meta2 / t2 as medgp_posterior_batch (meta2 may
 * be NULL for SE / SM and is range-checked for LMC-SM; a patient without points is allowed); no n > 2 guard, as there.  kind, psi, the
 * non-finite rule, the argument errors and the capacity rule as medgp_warp_nlml_grad; besides MEDGP_ERR_ARG for nq < 0 or nq > 64, a
 * non-finite zq entry, offsets that do not start at 0 or decrease, t2 (or, for LMC-SM, meta2) NULL with points, zmean and zvar not both
 * or neither NULL, quant without nq >= 1 and zq, lpd without y2.  The work rows are chunked within MEDGP_POSTERIOR_BUDGET_GB.  The
 * points of a patient with status[b] < 0 get NaN.  Every output pointer may be NULL.
 * A point's bits depend on the patient, theta, psi, kind and that point alone: not on the other points or their ORDER, the tile or
 * column it lands in, the launch chunk, or -- with the route pinned -- the batch-mates.
 * Supported range of the time stamps: |t| <= 2^14 h, as medgp_posterior_batch.  All pointers are HOST memory. */
int medgp_warp_posterior_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int32_t *kind,
                               const double *psi, const int64_t *offsets, const int32_t *meta2, const float *t2,
                               const float *y2 /* [M] or NULL */, int nq, const double *zq /* [nq] */, double *zmean,
                               double *zvar /* [M] */, double *quant /* [M][nq] */, double *lpd /* [M] */, int32_t *status);

/* Per-observation noise scales and Student-t robust training (kernels_hetero.h; the definition is tests/hetero_truth.py).
 * Every other call gives all observations of covariate d the noise variance sigma^2_d.  Here row i (covariate d = m_i; SE / SM: D = 1)
 * carries a scale s_i > 0: the mean of k monitor readings has s = 1 / k, a second device its own variance ratio, a flagged value a
 * large s.  With r jitter rounds the factored noise is N_i = (1 + r) sigma^2_d s_i (a jitter round adds the SCALED noise vector
 * again), K_s = K + diag(N), P = K_s^-1, alpha = P y:
 *   nlml   = 1/2 y^T alpha + 1/2 log|K_s| + 1/2 n log 2 PI                  (+ the priors on theta, as medgp_nlml_grad)
 *   grad_h = 1/2 tr((P - alpha alpha^T) dK_s / d theta_h): the usual lines for the covariance hypers; for the noise hyper of covariate d
 *            medgp_nlml_grad's line with s_i W_ii in the place of W_ii, sigma^2_d sum_{m_i = d} s_i W_ii
 *   resid_i = y_i - E f_i = N_i alpha_i,   fvar_i = var f_i = N_i - N_i^2 P_ii        (per training row, fp64)
 * status as medgp_nlml_grad (n <= 2: -1, else the jitter rounds).
 *
 * medgp_set_noise_scale makes scales resident: slot slots[k] gets scale[offsets[k] .. offsets[k + 1]), one per observation in the order
 * the patient was uploaded (offsets[0] = 0; the count must equal the patient's n).  scale == NULL drops the tables of the slots
 * (offsets is not read).  A scale must be finite and lie in [2^-40, 2^40], else MEDGP_ERR_ARG naming the index.  A later
 * medgp_set_patient[s] on a slot drops its table.  ONLY medgp_hetero_nlml_grad and medgp_hetero_posterior_batch read the tables (a slot
 * without one counts as all ones); EVERY OTHER CALL IGNORES THEM, medgp_robust_nlml_grad included (it takes scale0).  No device wait. */
int medgp_set_noise_scale(medgp_ctx *ctx, int nslots, const int32_t *slots, const int64_t *offsets,
                          const double *scale /* caller's row order; NULL drops the tables */);
/* The heteroscedastic nlml, its gradient (flag_grad = 1) and the row statistics, under the slots' resident scales.  resid and fvar are
 * packed by entry in the caller's row order (entry b owns sum_{b' < b} n_b' onward); each may be NULL; the rows of an entry with
 * status < 0 get NaN.  With all scales 1 (no table, or a table of ones) nlml, grad and status are bit-equal to medgp_nlml_grad's.
 * MEDGP_ERR_ARG for Q > 16 (as the warp calls), unknown bits in flag_grad, a slot without a patient; MEDGP_ERR_CAPACITY when the two
 * matrices of every entry and the call's vectors exceed the memory budget (split the call).  All pointers are HOST memory. */
int medgp_hetero_nlml_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, int flag_grad, double *nlml,
                           double *grad /* [nbatch][H] */, double *resid, double *fvar /* packed by entry, caller's row order, optional */,
                           int32_t *status);
/* The posterior at test points (m*_j, t*_j) under the slots' resident scales, with V_j = L^-1 k*_j, z = L^-1 y and an optional scale
 * s2[j] of the point's own noise (NULL: 1 for every point; 0: the latent f; finite, in [0, 2^40]):
 *   mean[j] = V_j^T z,   var[j] = k** - V_j^T V_j + sigma^2_{m*_j} s2[j]
 * fp64 outputs in the caller's point order; offsets / meta2 / t2 and their errors as medgp_posterior_batch; no n > 2 guard, as there;
 * mean and var both or neither NULL.  The points of a patient with status[b] < 0 get NaN. */
int medgp_hetero_posterior_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                                 const int32_t *meta2, const float *t2, const double *s2 /* [M] or NULL */, double *mean, double *var,
                                 int32_t *status);
/* Student-t observation noise by variational reweighting: eps_i | tau_i ~ N(0, sigma^2_d / tau_i), tau_i ~ Gamma(nu_d / 2, nu_d / 2),
 * q(tau_i) = Gamma(a_d, a_d s_i) with a_d = (nu_d + 1) / 2, so E tau_i = 1 / s_i.  With q(f) optimal for the given s the negative
 * evidence bound is
 *   J(theta, nu, s) = nlml_het(theta; s) + sum_i kappa(nu_{m_i}, s_i),   kappa(nu, s) = C(nu) + c (log s + 1 / s),   c = nu / 2,
 *   C(nu) = psi(a) / 2 - lgamma(a) + lgamma(c) + c log(a / c) - a - (psi(a) - log a) / 2,
 * J >= the exact Student-t nlml, and at fixed s dJ / dtheta is the heteroscedastic gradient exactly.  One E-step from a factorisation
 * at s is  e_i = (resid_i^2 + fvar_i) / sigma^2_{m_i},  s_i <- (nu_d + e_i) / (nu_d + 1).
 * The call starts from scale0 (packed by entry in the caller's row order, range as medgp_set_noise_scale; NULL = ones -- the resident
 * tables are NOT read), makes `sweeps` E-steps (0 .. 64) and evaluates obj = J, grad, resid and fvar at the last scales, which it
 * returns in `scale`: sweeps + 1 factorisations, queued without a host read-back in between.  sweeps = 0 with ones is the Gaussian nlml
 * plus sum_d n_d (C(nu_d) + c_d).  delta[b] = max_i |s_new - s_old| / s_new of the last E-step (0 with sweeps = 0).  nu: [nbatch][D]
 * (SE / SM: D = 1), finite and > 0, else MEDGP_ERR_ARG naming the index; nu is not learned here (medgp_amd.robust.select_nu scans a
 * grid in one call).  status[b]: the jitter rounds of the final evaluation, or -1 (n <= 2, or a factorisation that failed in ANY sweep);
 * such an entry's outputs are NaN and its batch-mates are unaffected.  Every output pointer may be NULL.  Errors and the capacity rule
 * as medgp_hetero_nlml_grad.  All pointers are HOST memory. */
int medgp_robust_nlml_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const double *nu /* [nbatch][D] */,
                           int sweeps /* 0..64 */, const double *scale0 /* packed, or NULL = ones */, int flag_grad, double *obj,
                           double *grad, double *scale, double *resid, double *fvar, double *delta, int32_t *status);

/* Rolling-origin forecasts: every test point predicted from a LEADING block of its patient's observations, all from ONE
 * factorisation per patient -- what the model says at time t from what was known before t.
 *   ref: core/gp_regression.cpp:128-214 (GP_Regression::predict), main_one_test.cpp:269-300 (the "past" training sets of the
 *        reference's test program), medgpc/evaluation/evals.py:7-51 (the scores computed from such predictions;
 *        medgp_amd/forecast.py restates them)
 * For a lower-triangular L the first p rows of V = L^-1 K* are L[0:p,0:p]^-1 K*[0:p], and L[0:p,0:p] is the factor of the
 * leading block K[0:p,0:p]: with z = L^-1 y,
 *   mean_j = sum_{k < p_j} V[k,j] z[k],   var_j = k** - sum_{k < p_j} V[k,j]^2 + sigma^2_{meta2_j}      (kernels_forecast.h).
 * nbatch, slots, theta, offsets, meta2, t2 and status mean exactly what they mean for medgp_posterior_batch: one factorisation
 * per patient, no n > 2 guard, status[b] = jitter rounds or -1, meta2 may be NULL for SE / SM, an empty range of points is allowed.
 *   prefix[j] in [0, n_b] (b = the patient of point j): point j is predicted from the FIRST prefix[j] observations of patient b
 *     in the caller's observation order, the order given to medgp_set_patient[s].  The library does not look at the time stamps
 *     to decide what is "earlier": a caller who uploads in time order gets forecasts, any other order gives the prediction from
 *     that leading subset.  (A patient not uploaded grouped by output is factored on its caller-order copy.)  A value outside
 *     the range: MEDGP_ERR_ARG before any device work.  prefix == NULL means prefix[j] = n_b: conditioning on all data, like
 *     medgp_posterior_batch, but in the caller's order.
 *   mean[j], var[j]: GP_Regression::predict applied to the training set obs[0:prefix[j]], the noise of the test covariate added
 *     once.  prefix[j] == 0 is the prior: mean exactly 0.0f, var = float(k** + sigma^2).
 *   y2, lpd: both NULL or both given (else MEDGP_ERR_ARG).  lpd[j] = -1/2 log(2 pi var_j) - 1/2 (y2_j - mean_j)^2 / var_j, formed
 *     in fp64 from the fp64 mean and variance before those are rounded to float, with the context's pi (medgp_set_pi) as
 *     medgp_loo_batch.  Summed over a patient's one-step-ahead points it is the prequential log score.
 * After k jitter rounds every quantity is that of the matrix that was factored, K + k diag(sigma^2), restricted to the prefix
 * (the rule of the posterior and LOO calls); a refit of the prefix alone might have needed fewer rounds.  The points of a
 * patient with status[b] < 0 get NaN mean, var and lpd.  There is NO per-covariate decomposition (parts): it needs alpha of
 * every prefix, which this route does not form.  A call whose per-entry matrices exceed the memory budget fails with
 * MEDGP_ERR_CAPACITY, like medgp_posterior_batch; the work rows are chunked within MEDGP_POSTERIOR_BUDGET_GB.
 * A point's outputs depend on the patient, theta, the point and its prefix alone: not on the other points of the call, their
 * order, the tile a point lands in, the launch chunk, or -- with the route pinned -- the batch-mates.  var is non-increasing
 * in prefix[j], exactly.
 * Accuracy (tests/test_forecast_gpu.py, against a refit of every prefix, tests/forecast_ref.py): mean and var within the
 * project's bar of 2 fp32 ulps of max(|ref|, 1e-3 S); lpd within B max(1, |ref|), B = 50 x the spread of the two fp64
 * restatements recorded in tests/golden/forecast_lpd_spread.json (2.8e-13, so B = 1.4e-11).  The tests print the worst
 * observed errors of every case (pytest -s).
 * Supported range of the time stamps: |t| <= 2^14 h, of the training observations AND of the test points, as medgp_posterior_batch.
 * mean and var keep the 2-ulp bar over the whole range.  B = 1.4e-11 holds NEAR THE ORIGIN (|t| <= 200 h, periods of 12 h and
 * more) only: lpd is an fp64 output of K and K* formed from cos / sin (w t) tables and loses |w t| eps with them.  An fp64 program
 * that forms its cosines from such tables is off, relative to max(1, |ref|), by 3.7e-13 (|t| <= 200 h), 2.7e-12 (2^10 h) and
 * 4.4e-11 (2^14 h) at a period of 1 h, by 4.1e-12 at 2^14 h and 12 h, by 5.8e-13 at 2^14 h and 72 h; with 17 components of 1 h,
 * 4.3e-12, 4.3e-11 and 2.4e-10 (tests/golden/time_shift_spread.json, tests/test_time_shift.py).  Away from the origin the bound is
 * max(B, 50 x that table error); tests/test_time_shift_gpu.py holds the device to it at -2^14, 2^10 and 2^14 h (the device's
 * errors there equal the table program's to two digits).
 * All pointers are HOST memory. */
int medgp_forecast_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                         const int32_t *meta2, const float *t2, const int32_t *prefix, const float *y2,
                         float *mean, float *var, double *lpd, int32_t *status);

/* The h-hours-ahead forecast score as a training objective, with its gradient in the hyper-parameters: what medgp_forecast_batch
 * reports (the log predictive density of each observation given what was known some hours before it), made optimisable.  The
 * reference evaluates on such forecasts (medgpc/evaluation/evals.py, main_one_test.cpp:269-300) but has no such output; the
 * definition is the long-double restatement in tests/forecast_grad_truth.py.  Observations are in the caller's upload order,
 * 0 .. n-1; K is the matrix that is factored, noise included.  Scored observation i has a history length p_i in [0, i]:
 *   a_i = K[0:p,0:p]^-1 K[0:p,i],  mean_i = a_i^T y[0:p],  var_i = K[i,i] - K[0:p,i]^T a_i,  r_i = y_i - mean_i,
 *   lpd_i = -1/2 log(2 pi var_i) - 1/2 r_i^2 / var_i,        J = - sum_{i scored} lpd_i,
 * lpd_i being exactly medgp_forecast_batch's lpd of a test point placed at observation i (meta2 = meta_i, t2 = t_i, y2 = y_i,
 * prefix = p_i).  With u_i = [-a_i on [0, p_i) | 1 at i | 0 elsewhere] and beta_i = [K[0:p,0:p]^-1 y[0:p] on [0, p_i) | 0],
 *   dJ / d theta_h = 1/2 tr(W_fc dK / d theta_h),
 *   W_fc = sum_i [ g_i u_i u_i^T - e_i (beta_i u_i^T + u_i beta_i^T) ],   g_i = (1 - r_i^2 / var_i) / var_i,   e_i = r_i / var_i:
 * the marginal-likelihood gradient with W_fc in the place of W.  Everything comes from ONE factorisation per patient
 * (kernels_forecast_grad.h).  p_i = i for every i is the chain rule of the likelihood: J is the nlml of medgp_nlml_grad without
 * a prior and W_fc = K^-1 - alpha alpha^T.
 * nbatch, slots, theta, status as medgp_loo_grad (no n > 2 guard; status[b] = jitter rounds or -1).
 *   offsets[nbatch + 1] index prefix: patient b owns offsets[b + 1] - offsets[b] = n_b values, in the caller's observation order.
 *   prefix[i] = -1: observation i is not scored; otherwise 0 <= prefix[i] <= i.  A value outside that range, offsets[0] != 0 or a
 *     range length different from n_b: MEDGP_ERR_ARG before any device work.  prefix == NULL means prefix[i] = i, everything
 *     scored (offsets may then be NULL too).  The library does not look at the time stamps to decide what is "earlier"
 *     (medgp_forecast_batch's rule; medgp_amd.forecast.training_prefix builds the table from times and a horizon).  A patient not
 *     uploaded grouped by output is factored on its caller-order copy; the gradient's tile reductions then run against the
 *     grouped copy, which the operands were stored for.
 *   obj[b] = J plus the prior term exactly as medgp_nlml_grad adds it for that slot; a patient without a scored observation has
 *     J = 0 and the prior's gradient alone.  log 2 pi uses the context's pi (medgp_set_pi).
 *   grad[b * H ..], flag_grad: as medgp_loo_grad (0 = the objective only, the same bits of obj; any other bit, or grad == NULL with
 *     flag_grad = 1: MEDGP_ERR_ARG before any device work).
 * After k jitter rounds every quantity is that of the matrix that was factored, K + k diag(sigma^2), and the noise gradient is
 * not scaled by 1 + k.  A patient with status[b] < 0 gets NaN obj and grad.  All three covariance families; Q <= 16 only: Q > 16
 * returns MEDGP_ERR_ARG, and MEDGP_V0 is not honoured by this call.  A call whose per-entry matrices exceed the memory budget
 * fails with MEDGP_ERR_CAPACITY (no memory waves); a gradient call holds one more ldn^2 matrix per entry (T) in a buffer of its own.
 * With the route pinned a patient's obj and grad bits do not depend on its batch-mates or their order: no atomics, every sum in a
 * fixed order.  medgp_get_factor is REFUSED afterwards (MEDGP_ERR_ARG): the call overwrites L and L^-1 with its operands.
 * Supported range of the time stamps: |t| <= 2^14 h (medgp_set_patient).  obj and grad are held to the fp64 budget of
 * tests/forecast_grad_truth.py near the origin (|t| <= 200 h); K and the gradient factors come from the cos / sin (w t_i) tables
 * and lose |w t| eps with them away from it, as medgp_loo_grad's.
 * All pointers are HOST memory. */
int medgp_forecast_grad(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                        const int32_t *prefix, int flag_grad, double *obj, double *grad, int32_t *status);

/* Posterior of the latent SLOPE at the test points, next to the posterior of the value: is the covariate rising or falling at t*,
 * how fast, and how sure is the model.  The derivative of a GP is a GP, and the SE / SM / LMC-SM covariances are differentiable
 * in closed form.
 *   ref: core/gp_regression.cpp:128-214 (GP_Regression::predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
 * The reference has no such output; the definition is the fp64 / long-double restatement of tests/trend_ref.py.
 * Component q is k_q(tau) = cos(w_q tau) exp(-c_q tau^2), w_q = 2 pi mu_q, c_q = 2 (pi v_q)^2 (SE: w = 0, c = 1 / (2 l^2),
 * B = sf^2).  For a test point (m*, t*) and a training observation (m_i, t_i), tau = t* - t_i:
 *   K*'[i]  = sum_q B_q[m_i, m*] (-w_q sin(w_q tau) - 2 c_q tau cos(w_q tau)) exp(-c_q tau^2)     (d/dt* of the cross Gram)
 *   k''**   = sum_q B_q[m*, m*] (w_q^2 + 2 c_q)                                                   (prior variance of f')
 *   V = L^-1 K*,  V' = L^-1 K*',  z = L^-1 y
 *   dmean[j] = V'^T z            posterior mean of f'_{m*}(t*), per hour, in the units of y
 *   dvar[j]  = k''** - sum V'^2   posterior variance of the LATENT slope (a noisy observation has no derivative: no sigma^2)
 *   cross[j] = - sum V V'         posterior cov(f(t*), f'(t*)); the prior term k'(0) is exactly 0.  May be NULL.
 *   mean[j], var[j]              exactly those of medgp_posterior_batch(parts = NULL) on the same call, bit for bit (var carries
 *                                sigma^2_{m*} once)
 * nbatch, slots, theta, offsets, meta2, t2, mean, var and status mean exactly what they mean for medgp_posterior_batch: one
 * factorisation per patient, no n > 2 guard, status[b] = jitter rounds or -1, meta2 may be NULL for SE / SM, an empty range of
 * points is allowed.  dmean and dvar are required (NULL: MEDGP_ERR_ARG before any device work).  The points of a patient with
 * status[b] < 0 get NaN in all five outputs.  After k jitter rounds every quantity is that of the matrix that was factored,
 * K + k diag(sigma^2) (the rule of the posterior, LOO and forecast calls).
 * Supported range of the time stamps: |t| <= 2^14 h, of the training observations (medgp_set_patient) AND of the test points: the
 * slope is formed from the same cos / sin (w t_i) tables as the value, sin(w (t_i - t*)) = sn_i cos(w t*) - cs_i sin(w t*).
 * A point's five outputs depend on the patient, theta and the point alone: not on the other points of the call, their order, the
 * tile or column a point lands in, the launch chunk, or -- with the route pinned -- the batch-mates.
 * The points go in tiles of 32 per workgroup: the 64 columns of the forward solve on fp64 MFMA are the value and the slope
 * column of every point (kernels_trend.h).  Work memory per launch within MEDGP_POSTERIOR_BUDGET_GB; a call whose per-entry
 * matrices exceed the memory budget fails with MEDGP_ERR_CAPACITY, like medgp_posterior_batch.
 * Accuracy: tests/test_trend_gpu.py holds all five outputs to the project's bar of 2 fp32 ulps of max(|ref|, 1e-3 S).
 * All pointers are HOST memory. */
int medgp_trend_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                      const int32_t *meta2, const float *t2, float *mean, float *var,
                      float *dmean, float *dvar, float *cross, int32_t *status);

/* Posterior of every spectral COMPONENT of the latent function at the test points: which part of the model a prediction comes from.
 * The SE / SM / LMC-SM prior is a sum of Q independent latent components, f = sum_q f_q, each with its own period 1 / mu_q and
 * envelope scale; the posterior of every f_q at a test point is in closed form from the factorisation the other calls make.
 *   ref: core/gp_regression.cpp:128-214 (GP_Regression::predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
 * The reference has no such output; the definition is the fp64 / long-double restatement of tests/components_ref.py.
 * Component q is k_q(tau) = cos(w_q tau) exp(-c_q tau^2), w_q = 2 pi mu_q, c_q = 2 (pi v_q)^2 (SE: Q = 1, w = 0, c = 1 / (2 l^2),
 * B = sf^2; SM: B_q = the 1 x 1 weight).  For a test point j = (m*, t*) and a training observation (m_i, t_i), tau = t* - t_i:
 *   K*_q[i]     = B_q[m_i, m*] k_q(tau)                  (sum_q K*_q = K* of medgp_posterior_batch)
 *   V_q = L^-1 K*_q,  z = L^-1 y                         (L: the ONE factor of the call, after its jitter rounds)
 *   cmean[j*Q + q]         = V_q^T z                              posterior mean of f_q at (m*, t*)
 *   ccov[(j*Q + q)*Q + r]  = delta_qr B_q[m*, m*] - V_q^T V_r     posterior covariance of (f_q, f_r) at the point; LATENT: no sigma^2
 *   cvar[j*Q + q]          = ccov[(j*Q + q)*Q + q]
 * In exact arithmetic sum_q cmean = mean and sum_qr ccov + sigma^2_{m*} = var of medgp_posterior_batch.  The mean of a band S of
 * components is sum_{q in S} cmean, its variance sum_{q, r in S} ccov (medgp_amd/components.py).
 * nbatch, slots, theta, offsets, meta2, t2 and status mean exactly what they mean for medgp_posterior_batch: one factorisation per
 * patient, no n > 2 guard, status[b] = jitter rounds or -1, meta2 may be NULL for SE / SM, an empty range of points is allowed, j
 * counts the points of the call (offsets[b] + i).  cmean and cvar are required (NULL: MEDGP_ERR_ARG before any device work).  ccov
 * may be NULL: the pair sums are not formed then.  Both triangles of ccov are written and are exactly symmetric, its diagonal has the
 * bits of cvar, an off-diagonal is written as 0.0 - sum.  All three covariance families, 1 <= Q <= 64: a point's Q columns must fit
 * one 64-column tile, Q > 64 is MEDGP_ERR_ARG.  The points of a patient with status[b] < 0 get NaN in all three outputs.  After k
 * jitter rounds every quantity is that of the matrix that was factored, K + k diag(sigma^2) (the rule of the other inference calls).
 * Supported range of the time stamps: |t| <= 2^14 h, of the training observations AND of the test points, as medgp_trend_batch:
 * cos(w_q (t_i - t*)) is formed from the tables cos / sin (w_q t_i) and cos / sin (w_q t*).
 * A point's outputs depend on the patient, theta and the point alone: not on the other points of the call, their order, the tile or
 * the columns a point lands in, the launch chunk, or -- with the route pinned -- the batch-mates.  Every sum runs in fixed row order
 * on one thread.
 * The points go in tiles of 64 / Q per workgroup: the 64 columns of the forward solve on fp64 MFMA are the Q component columns of
 * every point (kernels_components.h).  Work memory per launch within MEDGP_POSTERIOR_BUDGET_GB; a call whose per-entry matrices
 * exceed the memory budget fails with MEDGP_ERR_CAPACITY, like medgp_posterior_batch.
 * Accuracy: tests/test_components_gpu.py holds cmean, cvar and ccov to the project's bar of 2 fp32 ulps of max(|ref|, 1e-3 S), S the
 * patient's largest |ref| of the quantity (for ccov over the whole m x Q x Q block).
 * All pointers are HOST memory. */
int medgp_components_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta, const int64_t *offsets,
                           const int32_t *meta2, const float *t2, float *cmean, float *cvar, float *ccov, int32_t *status);

/* Posterior of LINEAR FUNCTIONALS of the latent function: the mean over a window, the change over an interval, the contrast of two
 * covariates, a time-weighted exposure.  Each is g = sum_k a_k f_{m_k}(t_k) over a list of terms (m_k, t_k, a_k), and its posterior is
 * a Gaussian in closed form from the factorisation the other calls make -- with ONE solve column per functional (linearity:
 * V_g = L^-1 (K* a)), no m x m covariance block, and every difference formed in fp64.
 *   ref: core/gp_regression.cpp:128-214 (GP_Regression::predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
 * The reference has no such output; the definition is the fp64 / long-double restatement of tests/functional_ref.py.
 * Component q is k_q(tau) = cos(w_q tau) exp(-c_q tau^2), w_q = 2 pi mu_q, c_q = 2 (pi v_q)^2 (SE: Q = 1, w = 0, c = 1 / (2 l^2),
 * B = sf^2; SM: B_q = the 1 x 1 weight).  For a training observation (m_i, t_i), tau = t_k - t_i, L and z = L^-1 y of the ONE factor of
 * the call (after its jitter rounds):
 *   K*_g[i]  = sum_k a_k sum_q B_q[m_i, m_k] k_q(tau)                      the terms in the caller's order
 *   V_g      = L^-1 K*_g
 *   fmean[f] = V_g^T z                                                     posterior mean of g
 *   q_g      = sum_k sum_l a_k a_l sum_q B_q[m_k, m_l] k_q(t_k - t_l)      prior variance of g
 *   fvar[f]  = q_g - sum_i V_g[i]^2                                        posterior variance of g; LATENT: no sigma^2 anywhere
 * Layout: patient b owns the functionals [foffsets[b], foffsets[b + 1]) of the call (foffsets: nbatch + 1 values), functional f owns the
 * terms [toffsets[f], toffsets[f + 1]) (toffsets: F + 1 values, F = foffsets[nbatch]) of meta2 / t2 / weight.  foffsets[0] == 0,
 * toffsets[0] == 0, both non-decreasing.  A patient without functionals is allowed; a functional without terms is allowed and gets
 * exactly 0.0f / 0.0f.  At most 2^31 - 65 functionals and 2^31 - 1 terms per call.
 * nbatch, slots, theta and status mean exactly what they mean for medgp_posterior_batch: one factorisation per patient, no n > 2 guard,
 * status[b] = jitter rounds or -1; after k jitter rounds every quantity is that of the matrix that was factored, K + k diag(sigma^2).
 * meta2 may be NULL for SE / SM and is range-checked for LMC-SM, as the posterior call's.  MEDGP_ERR_ARG before any device work, with
 * nothing written: fmean or fvar NULL; weight, t2, toffsets or foffsets NULL (whatever the counts); meta2 NULL for LMC-SM; offsets that
 * do not start at 0 or decrease.  The functionals of a patient with status[b] < 0 get NaN in both outputs.  fvar is written as computed:
 * no clamp (a functional the data determine to rounding, or a contrast of a point with itself, may come out as a tiny negative number).
 * Supported range of the time stamps: |t| <= 2^14 h, of the training observations AND of the terms, as medgp_trend_batch: K*_g is formed
 * from the tables cos / sin (w_q t_i) and cos / sin (w_q t_k) (one sincos per term and q, once per call).  q_g is formed from the time
 * differences t_k - t_l themselves, in fp64: the small prior variance of a change score over a short interval does not inherit the
 * |w t| eps of the tables.
 * A functional's two outputs depend on the patient, theta and its own term list in the caller's order alone: not on the other
 * functionals of the call or their order, the tile or column it lands in, the launch chunk, or -- with the route pinned -- the
 * batch-mates.  Every sum has a fixed order that depends on the functional alone (terms in the caller's order, q inside; rows in
 * order).  REORDERING the terms of a functional may move the last bits of its outputs.
 * The functionals go in tiles of 64 per workgroup: the 64 columns of the forward solve on fp64 MFMA are 64 functionals
 * (kernels_functional.h); the columns of a tile may have different term counts, the caller's order is kept.  Work memory per launch
 * within MEDGP_POSTERIOR_BUDGET_GB; a call whose per-entry matrices exceed the memory budget fails with MEDGP_ERR_CAPACITY, like
 * medgp_posterior_batch.  All three covariance families, any Q the context accepts.
 * Out of scope: slope terms (f' inside a functional; medgp_trend_batch gives the slope at a point), the covariance BETWEEN two
 * functionals (medgp_posterior_joint_batch on the nodes gives it), and observation noise (g is a functional of the latent f: add the
 * noise of a future measurement on the caller's side).  medgp_functional_joint_batch below gives that covariance from the same solve
 * columns, without the m x m block of the nodes.
 * Accuracy: tests/test_functional_gpu.py holds fmean and fvar to the project's bar of 2 fp32 ulps of max(|ref|, 1e-3 S), S the
 * patient's largest |ref| of the quantity over its functionals, and fvar <= q_g (1 + 2^-22).
 * All pointers are HOST memory. */
int medgp_functional_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta,
                           const int64_t *foffsets,   /* nbatch + 1: functionals of patient b are [foffsets[b], foffsets[b+1]) */
                           const int64_t *toffsets,   /* F + 1 (F = foffsets[nbatch]): terms of functional f are [toffsets[f], toffsets[f+1]) */
                           const int32_t *meta2, const float *t2, const double *weight,   /* per term; meta2 may be NULL for SE / SM */
                           float *fmean, float *fvar, int32_t *status);

/* JOINT posterior of a patient's linear functionals: medgp_functional_batch plus the posterior covariance BETWEEN the functionals of
 * each patient -- what a joint statement about several summaries needs ("the 24 h mean of A is falling AND that of B"; the variance
 * of the contrast g_A - g_B is v_A + v_B - 2 c_AB), what composes further functionals on the host without another call, and what
 * experimental design needs: with single-term `point` functionals as candidate measurements among the targets, the block holds
 * targets x candidates and candidates x candidates (medgp_amd/design.py: expected variance reduction, rank-1 conditioning, greedy
 * picks).
 *   ref: core/gp_regression.cpp:128-214 (GP_Regression::predict), kernel/c_kernel_LMC_SM.cpp:329-372 (cross Gram)
 * The reference has no such output; the definition is tests/functional_joint_ref.py.  With V_f = L^-1 K*_f of medgp_functional_batch:
 *   fcov[f, g] = q_fg - V_f^T V_g                                                  posterior covariance of (g_f, g_g)
 *   q_fg       = sum_{k in f} sum_{l in g} a_k a_l sum_q B_q[m_k, m_l] k_q(t_k - t_l)      their prior covariance
 * LATENT: no sigma^2 anywhere, and no clamp.  The arguments, the limits, the MEDGP_ERR_ARG cases, the jitter rule (after k rounds
 * every quantity is that of K + k diag(sigma^2)) and the supported range of the time stamps are those of medgp_functional_batch.
 * fmean and fvar are that call's outputs BIT FOR BIT (the same kernel launches on the same tiles).  fcov, fmean and fvar are all
 * required: NULL is MEDGP_ERR_ARG before any device work.
 * Layout of fcov: with F_b = foffsets[b + 1] - foffsets[b], patient b's block starts at fcov + sum_{a < b} F_a^2 and is F_b x F_b,
 * row-major, both triangles written.  F_b == 0 is allowed.  Only the lower triangle is computed, the upper one is mirrored from the
 * same float: fcov is exactly symmetric.  Its diagonal is not taken from the product: fcov[f, f] has the bits of fvar[f].  A functional
 * without terms gives a row and a column of exact 0.0f.  A patient with status[b] < 0 gets NaN in all three outputs.
 * q_fg is formed like q_g, from the time differences t_k - t_l themselves in fp64 (no cos / sin (w t) tables): the covariance of two
 * short change scores is as small as their variances.  For f > g in the caller's numbering the terms of f run in the outer loop and
 * those of g inside, both in the caller's order, q innermost; V_f^T V_g runs over the rows in order.
 * An element depends on the patient, theta, the two term lists and WHICH OF THE TWO COMES FIRST in the call: not on the other
 * functionals, the tile or column either lands in, the launch chunk, or -- with the route pinned -- the batch-mates.  REORDERING the
 * terms of a functional may move the last bits of its outputs, and so may SWAPPING THE ORDER of two functionals those of their
 * covariance (f > g decides which term list is the outer loop).
 * Memory: the call is cut into launch chunks of WHOLE patients within MEDGP_POSTERIOR_BUDGET_GB; the V of all tiles of a patient
 * (ceil(F_b / 64) x n_pad x 64 doubles) and its F_b^2 floats are resident together; no fp64 copy of the block is kept, because nothing
 * is factored.  A single patient beyond the budget fails with MEDGP_ERR_CAPACITY, as the joint posterior's; so does a call whose
 * per-entry matrices exceed the memory budget.
 * fcov is positive semi-definite in exact arithmetic only (empty and degenerate functionals give zero eigenvalues, rounding makes them
 * tiny negative ones): it is not factored here.
 * Out of scope: slope terms inside functionals, sampling from (or factorising) fcov, and a rectangular targets x candidates form (put
 * both lists into one call and slice the block).
 * Accuracy: tests/test_functional_joint_gpu.py holds fmean, fvar and fcov to the project's bar of 2 fp32 ulps of max(|ref|, 1e-3 S),
 * S the patient's largest |ref| of the quantity (for fcov over its whole F x F block).
 * All pointers are HOST memory. */
int medgp_functional_joint_batch(medgp_ctx *ctx, int nbatch, const int32_t *slots, const double *theta,
                                 const int64_t *foffsets, const int64_t *toffsets,
                                 const int32_t *meta2, const float *t2, const double *weight,
                                 float *fmean, float *fvar,
                                 float *fcov,   /* sum_b F_b^2: patient b's F_b x F_b block, row-major */
                                 int32_t *status);

/* Cohort statistics, the step after training: for each of nseries independent sample series
 * (series s = data[off[s] .. off[s] + cnt[s])) the Gaussian kernel density estimate with Silverman's bandwidth evaluated AT the
 * samples, and its "mode": weighted != 0: sum x dens / sum dens; weighted == 0: the sample with the largest density (first one).
 * Replaces compute_kde + compute_mode, ref: medgpc/clustering/mode_estimate.py:438-450 (statsmodels KDEUnivariate, kernel "gau",
 * bw "silverman"), as called per nugget / per cluster mu, v / per element of the aggregated B matrices by
 * output_mode_LMC_SM (ref: :277-279, :339-351, :410-413).  One-shot call on `device`, host arrays in and out, no context.
 * status[s]: 0 ok, -1 when the reference's fit would raise (n < 2, non-finite sample, zero bandwidth); mode[s] is NaN then.
 * bw (the bandwidths) and kernel_ms (HIP-event time of the kernel) may be NULL.  Errors: medgp_last_error(NULL). */
int medgp_kde_mode(int device, int nseries, const int64_t *off, const int32_t *cnt, const double *data, int weighted,
                   double *mode, double *bw, int32_t *status, double *kernel_ms);
/* The same with the density of series s evaluated on its own grid test[toff[s] .. toff[s] + tcnt[s]) (tcnt[s] == 0: at the
 * samples, as above); the mode is then taken over the grid points.  This is how output_mode_SE evaluates the length-scale
 * (ref: mode_estimate.py:54-57) and output_mode_SM the period / length-scale densities (ref: :170-184): 100001-point grids,
 * arg-max mode.  toff / tcnt / test are all NULL or all given. */
int medgp_kde_mode_at(int device, int nseries, const int64_t *off, const int32_t *cnt, const double *data, const int64_t *toff,
                      const int32_t *tcnt, const double *test, int weighted, double *mode, double *bw, int32_t *status,
                      double *kernel_ms);

/* Kernel clustering, the step between training and the mode kernel: EM for full-covariance Gaussian
 * mixtures on n points of dimension d, nruns independent runs in one call, each from its own start.  Replaces what scikit-learn's
 * GaussianMixture(covariance_type='full', n_init, max_iter) computes inside the reference's run_sklearn_gmm, ref:
 * medgpc/clustering/cluster.py:23-46 -- the restarts of every K = 1 .. Q are the runs; the selection (largest lower bound per K,
 * smallest BIC over K) is medgp_amd/clustering.py's.  There is no random generator on the device: run r starts from the hard labels
 * label0[r, i] in [0, k[r]) (one-hot responsibilities, then one M-step; a class may be empty), where scikit-learn starts from an
 * unseeded k-means.  The definition the kernels are held to is tests/gmm_ref.py:
 *   M-step: n_k = sum_i r_ik + 10 eps, w_k = n_k / n, mu_k = sum r_ik x_i / n_k, S_k = sum r_ik (x_i - mu_k)(x_i - mu_k)^T / n_k +
 *           reg_covar I, L_k = chol(S_k); a pivot <= 0 or NaN fails the run.
 *   E-step: log p_ik = -1/2 (d log 2 pi + |L_k^-1 (x_i - mu_k)|^2) - sum log diag L_k + log w_k, lse_i = logsumexp_k,
 *           r_ik = exp(log p_ik - lse_i), lb = mean_i lse_i.
 *   Loop:   it = 1 .. max_iter: E-step, M-step, change = lb - previous lb (-inf at first); converged when |change| < tol.
 *   After:  one E-step at the final parameters: assign = first arg max_k r_ik, bic = -2 n mean lse + (K d (d + 1) / 2 + K d + K - 1) log n.
 * Limits: 2 <= n, 1 <= d <= 80, 1 <= k[r] <= min(16, n), 1 <= nruns <= 65535, max_iter >= 1, tol >= 0, reg_covar >= 0; anything else is
 * MEDGP_ERR_ARG.  The call holds nruns * kmax * n responsibilities and at most 32 d x d partial sums per (run, component) on the
 * device at once: beyond MEDGP_GMM_BUDGET_GB (default 8) it fails with MEDGP_ERR_CAPACITY before any device work.
 * Outputs, kmax = max_r k[r]: lower_bound[r] the loop's last lb; status[r] 1 converged, 0 max_iter reached, -1 failed; n_iter[r] the
 * iterations run; weights / means / covs of the components (entries beyond a run's K are zero), assign[r, i].  A failed run has NaN
 * lower_bound, bic, weights, means and covs and assign -1; it does not fail the call.  weights, means, covs, assign and kernel_ms (HIP-event
 * time from the first to the last launch) may be NULL.  A run's outputs are bit-identical whatever the other runs of the call are and
 * however often the host polls the runs' flags (MEDGP_GMM_POLL iterations, default 8).  One-shot call on `device`, host arrays in and
 * out, no context.  Errors: medgp_last_error(NULL). */
int medgp_gmm_fit(int device, int n, int d, const double *x /* [n*d] row-major */,
                  int nruns, const int32_t *k /* [nruns] */, const int32_t *label0 /* [nruns*n] */,
                  int max_iter, double tol, double reg_covar,
                  double *lower_bound, double *bic, int32_t *n_iter, int32_t *status /* [nruns] */,
                  double *weights /* [nruns*kmax] */, double *means /* [nruns*kmax*d] */,
                  double *covs /* [nruns*kmax*d*d] */, int32_t *assign /* [nruns*n] */, double *kernel_ms);

/* Route pinning.  By default the library picks the factorisation schedule of a call from the batch it is given (one workgroup per
 * patient in two shapes, or the multi-CU look-ahead schedule for few large patients): fastest, and every schedule meets the parity
 * bar, but the LAST BITS of a patient's results can then depend on how many batch-mates it had.  pinned != 0: every entry of every
 * call is factored by the one 8-wave single-workgroup kernel, so a patient's results are bit-identical whatever the batch -- what a
 * caller needs whose outputs must not depend on how patients were grouped into calls (medgp_test: a cohort run writes the same
 * bytes as one run per patient).  The reference has no such choice: one patient per process, ref: main_one_test.cpp:45-481. */
int medgp_pin_route(medgp_ctx *ctx, int pinned);

/* How the last medgp_nlml_grad* call was scheduled (diagnostics; round 5).  A call's entries are cut into size classes by their
 * number of 64-observation blocks, (2^(j-1), 2^j], and every class is given its own launch geometry and factorisation route, the way
 * the reference's job generator gives patients resources by size (ref: scripts/slurm_della.json:6-62,
 * medgpc/util/run_exp_generator.py:213-260).  Writes, largest class first and for at most max_classes classes: count[i] entries,
 * blocks[i] = 64-blocks of its largest entry, route[i] = 0 / 1 one workgroup per entry in the 4- / 8-wave shape, 2 the multi-CU
 * look-ahead schedule.  Returns the number of classes of the call (possibly > max_classes), or an error code. */
int medgp_last_plan(const medgp_ctx *ctx, int max_classes, int32_t *count, int32_t *blocks, int32_t *route);

/* block until all work queued on the context's stream is complete */
int medgp_synchronize(medgp_ctx *ctx);

/* ---- measurement hooks (bench.py roofline leg; no effect on results) ------------------------- */
/* enable = 1: bracket every kernel launch with HIP events on the launch stream; enable = 2 + k: only the launches of kernel k
   (medgp_profile_kernel_name) -- two events per step instead of two per launch (bench.py times its headline region this way:
   the events of all seven launches cost 1.6 % of a 512-patient step); enable = 0: off */
int medgp_profile_enable(medgp_ctx *ctx, int enable);
/* number of distinct kernels the library launches, and their names.  The table counts profile ENTRIES: the launches of k_components
   (medgp_components_batch) and of k_functional (medgp_functional_batch) are accounted under the entry "k_posterior", the one
   k_functional_prep launch per size class of that call under "k_prep", so the table and every kernel id in it stay what they were */
int medgp_profile_num_kernels(void);
/* The table of medgp_profile_num_kernels is frozen at its 23 entries (callers index it).  Kernels that get entries of their own
   since -- medgp_forecast_grad's k_fc_vec, k_fc_t, k_fc_scan, k_fc_qm, k_fc_tables, k_fc_wgrad -- are appended behind it: ids
   [medgp_profile_num_kernels(), medgp_profile_num_kernels_all()) are valid for medgp_profile_kernel_name, medgp_profile_read and
   medgp_profile_enable(2 + k) like the ids before them. */
int medgp_profile_num_kernels_all(void);
/* medgp_profile_num_kernels_all is pinned as well, at the 29 entries it had when medgp_forecast_grad added it (its callers compare
   the whole list).  Entries added since -- medgp_lgo_grad's k_lgo_vec (k_lgo_mask, k_lgo_prep and k_lgo_obj), k_lgo_inv, k_lgo_s,
   k_lgo_t, k_lgo_wgrad, medgp_fisher_vec's k_fisher_prep, k_fisher_kdot, k_fisher_t, k_fisher_wgrad, and medgp_hess_vec's k_hess_moments,
   k_hess_slabsum, k_hess_beta, k_hess_wgrad, k_hess_epilogue, and medgp_posterior_jvp_batch's k_pjvp_solve, k_pjvp_u, k_pjvp_dir (ids 43 to 45), and
   medgp_posterior_vjp_batch's k_pvjp_cot, k_pvjp_wgrad, k_pvjp_cross, k_pvjp_finish (ids 46 to 49; its k_slabsum and k_epilogue launches are
   accounted under "k_epilogue", its solve under "k_pjvp_solve"), and the baseline calls' k_mean_g, k_mean_small, k_mean_panel,
   k_mean_wgrad, k_mean_post (ids 50 to 54; their k_slabsum, k_epilogue and k_pjvp_solve launches likewise) -- are appended behind it: ids [medgp_profile_num_kernels_all(), medgp_profile_num_kernels_ext()) are valid
   in the same way.  A caller that wants every entry walks [0, medgp_profile_num_kernels_ext()) and does not assume its length. */
int medgp_profile_num_kernels_ext(void);
/* medgp_profile_num_kernels_ext is pinned in turn, at the 58 entries it had when the basis calls were added.  The warp calls' k_warp_z,
   k_warp_solve, k_warp_small, k_warp_post (ids 58 to 61; their k_wgrad, k_slabsum, k_epilogue and k_pjvp_solve launches are accounted
   under the existing entries) are appended behind it: ids [medgp_profile_num_kernels_ext(), medgp_profile_num_kernels_ext2()) are
   valid in the same way. */
int medgp_profile_num_kernels_ext2(void);
/* medgp_profile_num_kernels_ext2 is pinned in turn, at its 62 entries, and so is medgp_profile_kernel_name: it answers "" from id 62 on
   (callers test the end of the table that way).  The heteroscedastic calls' k_het_load, k_het_rows, k_het_estep, k_het_obj, k_het_post
   (ids 62 to 66; their k_wgrad, k_slabsum, k_epilogue and k_pjvp_solve launches are accounted under the existing entries) are appended
   behind it: ids [medgp_profile_num_kernels_ext2(), medgp_profile_num_kernels_ext3()) are valid for medgp_profile_read and
   medgp_profile_enable(ctx, 2 + id); medgp_profile_kernel_name_ext3 names every id below medgp_profile_num_kernels_ext3(). */
int medgp_profile_num_kernels_ext3(void);
const char *medgp_profile_kernel_name_ext3(int k);
const char *medgp_profile_kernel_name(int k);
/* synchronises, then returns accumulated milliseconds and launch count of kernel k since the
 * last medgp_profile_reset */
int medgp_profile_read(medgp_ctx *ctx, int k, double *ms_total, int64_t *launches);
int medgp_profile_reset(medgp_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
