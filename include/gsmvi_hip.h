/*
 * gsmvi_hip.h -- C ABI of the MI355X (gfx950) GSM / BaM update engine.
 *
 * The reference (modichirag/GSM-VI) has no FFI layer: its boundary for this path is the set of
 * pure Python callables listed below.  Each entry point here is what a binding for that callable
 * would bind; the Python mirror in gsm-vi_amd/ calls them through ctypes.
 *
 *   reference callable (file:line, relative to the reference tree)     ->  entry point
 *   gsmvi/gsm_numpy.py:27-55  gsm_update(samples, vs, mu0, S0)          ->  gsmvi_gsm_update_f64
 *   gsmvi/gsm.py:31-58        gsm_update (JAX twin)                     ->  gsmvi_gsm_update_f64
 *   examples/example_gsm_numpy.py:24-29  lp_g of the Gaussian target    ->  gsmvi_gaussian_score_f64
 *   gsmvi/gsm_numpy.py:116    np.random.multivariate_normal(mean,cov,B) ->  gsmvi_sample_f64 (+ gsmvi_potrf_f64)
 *   gsmvi/gsm_numpy.py:105,116 np.random.seed + standard-normal stream  ->  gsmvi_randn_f64 (counter-based)
 *   gsmvi/gsm_numpy.py:132-146 _check_goodness(cov)                     ->  gsmvi_potrf_f64 (info flag)
 *   jax.vmap(gsm_update) over K problems, D <= 64 (gsm.py:31-58)       ->  gsmvi_gsm_update_batched_f64
 *   gsm_numpy.py:77-129 fit of K problems (dense form), D <= 64         ->  gsmvi_gsm_fit_{init,step}_batched_f64
 *   (no reference twin; gsm_numpy.py:4-55 in factor form)   ->  gsmvi_gsm_factor_update_f64
 *   jax.vmap(bam_update) over K problems, D <= 64 (bam.py:31-114)      ->  gsmvi_bam_update_batched_f64
 *   bam.py:189-212 fit iteration of K problems (dense), D <= 64         ->  gsmvi_bam_fit_step_batched_f64
 *   monitors.py:83-125 KL monitor of K problems, D <= 64               ->  gsmvi_kl_draw_batched_f64, gsmvi_logq_batched_f64
 *   advi.py:31-45,69-73 ELBO gradient + optimiser step, K problems      ->  gsmvi_advi_step_batched_f64
 *   advi.py:80-86 initial (loc, scales), :23-27 scales -> covariance    ->  gsmvi_advi_init_batched_f64, gsmvi_advi_cov_batched_f64
 *   examples/example_gsm.py:34-35 a model's log_prob and jit(grad(.)) of it, K logistic regressions -> gsmvi_logistic_batched_f64
 *   examples/example_gsm.py:34-35 the same for K Poisson, probit or Gaussian regressions with offsets -> gsmvi_glm_batched_f64
 *   examples/example_gsm.py:34-35 the same for K such regressions on ONE design matrix, with observation weights -> gsmvi_glm_shared_batched_f64
 *   examples/example_gsm.py:34-35 the same for K multinomial logit (softmax) regressions of C classes -> gsmvi_softmax_batched_f64
 *   examples/example_gsm.py:34-35 the same for K cumulative-logit (ordinal) regressions of C ordered classes -> gsmvi_ordinal_batched_f64
 *   initializers.py:5-17 lbfgs_init (maximiser of lp, dense inverse-Hessian estimate), K problems -> gsmvi_lbfgs_step_batched_f64, gsmvi_lbfgs_hess_inv_batched_f64
 *   initializers.py:5-17 the same role by Newton rounds on the GLMs of examples/example_gsm.py:34-35 (no reference twin) -> gsmvi_glm_hessian_batched_f64, gsmvi_laplace_step_batched_f64,
 *   gsmvi_softmax_hessian_batched_f64, gsmvi_softmax_laplace_step_batched_f64 (the multinomial logit),
 *   gsmvi_glm_shared_hessian_batched_f64, gsmvi_laplace_shared_step_batched_f64 (the GLMs on one design matrix),
 *   gsmvi_negbin_hessian_batched_f64, gsmvi_negbin_laplace_step_batched_f64 (the negative binomial regressions),
 *   gsmvi_ordinal_hessian_batched_f64, gsmvi_ordinal_laplace_step_batched_f64 (the cumulative-logit regressions)
 *   initializers.py:5-17 the same role with a start picked by its ELBO along the L-BFGS path (Pathfinder; no reference twin) -> gsmvi_pathfinder_propose_batched_f64, gsmvi_pathfinder_select_batched_f64
 *   examples/example_gsm.py:34-35 the use of the fit: predictions and the held-out score of K fitted GLMs (no reference twin) -> gsmvi_glm_predict_batched_f64
 *   monitors.py:83-125 the role (is q_k close to its target?), per problem and comparable across problems: the Pareto-smoothed
 *   importance diagnostic of K fitted Gaussians (no reference twin)    ->  gsmvi_psis_batched_f64, gsmvi_psis_weights_batched_f64
 *   examples/example_gsm.py:34-35 the comparison of fitted models: the PSIS leave-one-out density of every observation of K fitted
 *   GLMs (no reference twin)                                           ->  gsmvi_psis_loo_batched_f64, gsmvi_psis_loo_tile
 *   the same for K fitted multinomial logit regressions (no reference twin) -> gsmvi_psis_loo_softmax_batched_f64, gsmvi_psis_loo_softmax_tile
 *   the same for K fitted negative binomial regressions (no reference twin) -> gsmvi_psis_loo_negbin_batched_f64, gsmvi_psis_loo_negbin_tile
 *   the same for K fitted cumulative-logit regressions (no reference twin) -> gsmvi_psis_loo_ordinal_batched_f64, gsmvi_psis_loo_ordinal_tile
 *   the same for K fitted GLMs on one design matrix, weighted (no reference twin) -> gsmvi_psis_loo_shared_batched_f64
 *   examples/example_gsm.py:34-35 the use of the fit for K fitted multinomial logit regressions: class probabilities and the held-out
 *   score from draws of q_k (no reference twin)                        ->  gsmvi_softmax_predict_batched_f64, gsmvi_softmax_predict_lds_bytes
 *   the same use for K fitted negative binomial regressions: log moments of the predictive count and the held-out score from
 *   draws of q_k (no reference twin)                                   ->  gsmvi_negbin_predict_batched_f64
 *   the same use for K fitted cumulative-logit regressions: class probabilities and the held-out score from draws of q_k
 *   (no reference twin)                                                ->  gsmvi_ordinal_predict_batched_f64, gsmvi_ordinal_predict_lds_bytes
 *   the use of the fit for K fitted GLMs on one design matrix: the GLM predictive on one shared set of new rows with per-problem
 *   row weights, the held-out score of K-fold cross-validation (no reference twin) -> gsmvi_glm_shared_predict_batched_f64
 *   gsmvi/bam.py:72-114       bam_lowrank_update(samples,vs,mu0,S0,reg) ->  gsmvi_bam_update_f64
 *   gsmvi/bam.py:31-69        bam_update(samples,vs,mu0,S0,reg)         ->  gsmvi_bam_update_f64 (same result, K6)
 *
 * Conventions
 *   - All matrices are row-major float64 in DEVICE memory; `ld*` are leading dimensions in elements.
 *   - Calls are asynchronous on `stream` (a hipStream_t passed as void*); nothing synchronises,
 *     so call sequences can be captured into a hipGraph.
 *   - Inputs are never modified; outputs must not alias inputs (reference updates are pure,
 *     gsm_numpy.py:47-55) unless an entry point says otherwise.
 *   - S0 must be symmetric (it is a covariance); the kernels read it once, by rows.
 *   - Every function returns a gsmvi_status; no C++ exception crosses the ABI.
 *   - One context per stream; calls on one context are not thread-safe (the reference is
 *     single-threaded: gsm_numpy.py:105 uses the global numpy RNG).
 */
#ifndef GSMVI_HIP_H
#define GSMVI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is compiled with -fvisibility=hidden and linked with an export list (csrc/exports.map): exactly the
 * functions declared between this push and its pop are visible (tests/test_abi.py compares `nm -D` with this file). */
#pragma GCC visibility push(default)

#define GSMVI_ABI_VERSION 1

typedef enum gsmvi_status {
    GSMVI_OK = 0,
    GSMVI_ERR_BAD_ARG = 1,    /* NULL pointer, non-positive size, ld < D, aliasing, ...            */
    GSMVI_ERR_HIP = 2,        /* a HIP runtime call failed; see gsmvi_last_error()                 */
    GSMVI_ERR_NO_DEVICE = 3,  /* no gfx950 device visible                                          */
    GSMVI_ERR_WORKSPACE = 4,  /* (D,B) exceeds what the context was created for                    */
    GSMVI_ERR_UNSUPPORTED = 5
} gsmvi_status;

typedef struct gsmvi_ctx gsmvi_ctx;   /* opaque: device id, workspace, launch heuristics */

int gsmvi_abi_version(void);
const char* gsmvi_status_string(int status);
/* Message of the last failing call on this host thread ("" if none). */
const char* gsmvi_last_error(void);
/* Number of HIP devices; GSMVI_ERR_NO_DEVICE (and *n = 0) when there is none. */
int gsmvi_device_count(int* n);

/* Workspace bytes a context allocates for problems up to (max_D, max_B). */
size_t gsmvi_workspace_bytes(int max_D, int max_B);
/* Creates a context on `device` with workspace for D <= max_D, B <= max_B. */
/* gsmvi_create / gsmvi_destroy leave the caller's current HIP device as they found it.  The compute entry points
 * never change the current device either: `stream` must belong to the context's device and that device must be
 * current when they are called (what torch.cuda.set_device / hipSetDevice in the calling loop guarantees). */
int gsmvi_create(gsmvi_ctx** out, int device, int max_D, int max_B);
int gsmvi_destroy(gsmvi_ctx* ctx);
/* Launch-heuristic knobs for tests and A/B measurements: "panel_kc" (split-K count of the panel products; <= 0 = auto),
 * "no_fast" (1 = force the guarded generic kernels), "direct_out" (0 = always product + finish pass), "update_sb",
 * "scalars_nt", "bam_full", "bam_kenq", "rider", "wide", "wide_kc", "gram_mt", "fork_min_D", "potrf_split_m", "chain_pair"
 * (0 = one launch per one-workgroup factorisation of the 128 < 2B <= 256 chain); round 5: "bam_basis" (1 = factor-form BaM in
 * the orthogonal basis [Vw; Zt], default; 0 = the round-4 basis [Vw; Zw]; 3 = as 1 but the 2B x 2B chain factors its first
 * diagonal block itself), "bam_hint_slack" (Newton-Schulz steps enqueued beyond the previous call's count, default 1),
 * "rider_direct_max_D" (largest D at which the panel product carrying the chain as its rider runs unsplit, default 2048),
 * "lowrank_kp" (64 = 64-row staging passes of BaM's low-rank update); round 6: "potrf_dag" (0 = one launch per block step),
 * "potrf_spin" (poll budget of a wait inside k_potrf_dag), "potrf_workers" (cap on its worker workgroups: tests of the ticket
 * order), "panel_w4_min_D"; "bam_batched_pad" (0 = the batched BaM kernel's LDS arrays at the unpadded row strides D, B; A/B
 * runs); "gsm_two_launch" (default 1: the dense GSM update at B in {16, 32}, D % 256 == 0, D <= 1024 with even leading
 * dimensions and 16-byte aligned arrays runs as two launches without the per-sample kernel; 0 = always three launches;
 * an explicit "panel_kc" also selects 256-row chunks for its product at D = 1024, where the default is two 512-row slabs);
 * round 9: "cov_fold_diag" (two-launch form: the diagonal leftover tiles of the covariance launch ride as third tiles in
 * two-tile workgroups instead of being workgroups of their own; 1 = where the two-tile workgroups alone fill the device,
 * i.e. D = 1024 on 256 CUs, default; 0 = never; 2 = at every two-launch shape; results are bit for bit the same);
 * round 10, both for the two-slab covariance launch (D = 1024, no explicit "panel_kc") and both with bit-identical results:
 * "cov_s0_last" (1 = the Sigma0 tile is the last load issued and the last one waited for, behind the staging and the MFMAs),
 * "cov_store_wt" (1 = Sigma' is stored write-through, where D * lds * 8 < 2^31; the lines do not stay in the L2);
 * "panel_qm_whole" (same route; 1 = the product leaves one (mu0 - x_b).g_b per sample instead of D / 16 pieces that every
 * covariance workgroup re-sums; another summation order, so mu and Sigma' move at rounding level; default 0);
 * round 12: "panel_stream" (the product launch of the same route, without "panel_qm_whole": 1 = every wave loads the part of
 * G that it multiplies, in two stages along K, and starts a stage's MFMAs behind that stage's loads alone, with no workgroup
 * barrier in front of the first MFMA; 4 = in four stages, 2 = as 1, for A/B runs; 0 = one load batch staged by the whole workgroup behind a
 * barrier; bit-identical results, no path bit: the timeline diagnostic's stamp words 4 - 7 of the product tell them apart);
 * round 13: "cov_diag_quad" (the covariance launch where the fold runs: no hosts -- D / 64 workgroups own the diagonal 64 x 64
 * blocks, three tiles on two staged column blocks, every other tile rides in a pair; 1 = where the fold runs by default on the
 * two-slab form with "cov_s0_last" and "cov_store_wt" on and "panel_qm_whole" off, default; 0 = the fold as it was; 2 = wherever
 * "cov_fold_diag" is not 0, for tests; bit-identical results, reported under GSMVI_PATH_COV_FOLD_DIAG);
 * round 14: "cov_wave_store" (wherever "cov_diag_quad" selects the quads: 1 = every wave of the covariance launch forms W =
 * Sigma0 + U for the 16 x 16 block it computed, stores it and mirrors it through a wave-private LDS buffer, with no workgroup
 * barrier behind the MFMAs, default; 0 = the store path through shared LDS buffers and three barriers; bit-identical results,
 * no path bit);
 * round 15: "kernarg_preload" (both launches of the two-launch form: 1 = entry points whose argument block begins with the 14
 * dwords that the first load batch takes, delivered in SGPRs with the wave (gfx950 kernel-argument preload; firmware without it
 * runs an equivalent prologue), the remaining arguments fetched behind the first vector loads, default; 0 = the entry points with
 * the ordinary argument block; the same kernel bodies, bit-identical results, no path bit: all 32 are taken);
 * diagnostics "timeline", "cov_dbg"
 * (see gsmvi_hip_debug.h). */
int gsmvi_set_tuning(gsmvi_ctx* ctx, const char* name, int value);

/*
 * GSM batch update (dense-covariance path).  Replaces gsmvi/gsm_numpy.py:27-55.
 *   X  (B x D, ldx)  samples            G  (B x D, ldg)  scores lp_g(X)
 *   mu0 (D)          current mean       S0 (D x D, lds0) current covariance (symmetric)
 *   mu  (D)          new mean           S  (D x D, lds)  new covariance
 * mu = mu0 + mean_b dmu_b ; S = S0 + mean_b (d_b d_b^T - e_b e_b^T), d_b = mu0 - x_b, e_b = d_b + dmu_b.
 * Three kernels: panel product SG = G S0 (fp64 MFMA), per-sample scalars, rank-2B update (fp64 MFMA).
 * For B in {16, 32}, D % 256 == 0, D <= 1024, even leading dimensions and 16-byte aligned arrays: TWO kernels -- the product
 * also leaves partial dots, the update forms its factor tiles itself (knob "gsm_two_launch"; GSMVI_PATH_GSM_TWO_LAUNCH).
 * At D = 1024 that product runs as two slabs of one 512-row chunk each (GSMVI_PATH_PANEL_CHUNK512) unless "panel_kc" is set
 * explicitly, which keeps 256-row chunks with that split ("panel_kc" = 4: four slabs).
 * PRECONDITION: S0 is symmetric (a covariance).  For D % 32 == 0 and B in {16, 32, 64} the update kernel reads only
 * the UPPER triangle of S0 and mirrors the result, so S comes out exactly symmetric; for other shapes the generic
 * kernel reads all of S0.  A non-symmetric S0 therefore gives shape-dependent results that differ from
 * gsm_numpy.py:50-53 (S0 + mean): use gsmvi_gsm_update_general_f64 for such an S0 (the Python drop-in gsm_update() does
 * so for host inputs it finds non-symmetric, and on request for device inputs).
 * One context per stream: calls on one gsmvi_ctx share its workspace and must not run concurrently.
 */
int gsmvi_gsm_update_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                         const double* X, int ldx, const double* G, int ldg,
                         const double* mu0, const double* S0, int lds0,
                         double* mu, double* S, int lds);

/*
 * The same update for an S0 that is not symmetric: the reference's literal semantics S = S0 + mean_b (...) with S0 g_b in
 * the per-sample stage (gsm_numpy.py:7,50-53) for ANY square S0.  Reads all of S0 (transposed panel product + the guarded
 * update kernel); the Python drop-in gsm_update(..., assume_symmetric=False) calls it.  Not a performance path.
 */
int gsmvi_gsm_update_general_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                                 const double* X, int ldx, const double* G, int ldg,
                                 const double* mu0, const double* S0, int lds0,
                                 double* mu, double* S, int lds);

/*
 * The same update in two stages, for the batch-sharded multi-GPU path (one process per GPU):
 *   local stage : for this rank's B_local samples, panel product + per-sample scalars; writes one
 *                 record per sample  rec[b] = [ d_b (D) | e_b (D) | dmu_b (D) ]  (d_b = mu0 - x_b,
 *                 dmu_b = mu_update of gsm_numpy.py:17, e_b = d_b + dmu_b) with row stride
 *                 ldrec >= gsmvi_gsm_record_len(D) = 3D rounded up to even.  Records of all ranks are
 *                 all-gathered (RCCL) by the caller;
 *   apply       : every replica applies the combined rank-2B update from all B records.
 * gsmvi_gsm_update_f64 == local stage with B_local = B followed by apply.
 */
int gsmvi_gsm_record_len(int D);
int gsmvi_gsm_local_stage_f64(gsmvi_ctx* ctx, void* stream, int D, int B_local,
                              const double* X, int ldx, const double* G, int ldg,
                              const double* mu0, const double* S0, int lds0,
                              double* rec, int ldrec);
int gsmvi_gsm_apply_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                        const double* rec, int ldrec, const double* mu0,
                        const double* S0, int lds0, double* mu, double* S, int lds);

/*
 * Batch-sharded update over RCCL in ONE call (one process per GPU; SURVEY 8(b): "RCCL-sharded variants taking an
 * ncclComm_t"): local stage on this rank's B_local samples -> ncclAllGather of the records (B_local *
 * gsmvi_gsm_record_len(D) doubles per rank, in place in rec_all) on `stream` -> combined rank-2B update applied by
 * every replica; replicas end bit-identical.  nccl_comm is an ncclComm_t (passed as void* so that this header does
 * not need rccl.h) created by the caller with the RCCL library loaded in its process; this library resolves
 * ncclAllGather from that instance at first use and does not link RCCL itself.  rec_all: caller-owned device buffer
 * of (B_local * nranks) x gsmvi_gsm_record_len(D) doubles.  B_local * nranks must fit the context's max_B.
 * Python callers use torch.distributed instead (gsm-vi_amd/dist.py::sharded_gsm_update), same two stage calls.
 */
int gsmvi_gsm_update_sharded_f64(gsmvi_ctx* ctx, void* stream, void* nccl_comm, int D, int B_local,
                                 const double* X_local, int ldx, const double* G_local, int ldg,
                                 const double* mu0, const double* S0, int lds0, double* rec_all,
                                 double* mu, double* S, int lds);

/*
 * The RCCL library the sharded entry points call into.  By default they resolve ncclAllGather / ncclCommCount /
 * ncclCommUserRank at first use from the RCCL instance already loaded in the process (falling back to librccl.so.1).  A
 * process that holds several RCCL copies (e.g. torch's bundled one beside the system one) passes the dlopen handle of the
 * copy that CREATED its communicators here, before the first sharded call; afterwards the choice is fixed.
 */
int gsmvi_set_rccl_library(void* dl_handle);

/*
 * The same update with the covariance sharded by ROW BLOCKS (the decomposition that divides
 * the HBM-bound passes by the number of GPUs).  A rank owns rows [row0, row0 + nrows) of S0 as an
 * nrows x D row-major block; X, G, mu0 are replicated.
 *   rows stage : SGcols (B x nrows, ldsg) = G S0rows^T, i.e. columns [row0, row0+nrows) of G S0 (S0 symmetric,
 *                gsm_numpy.py:7).  The caller all-gathers the column slices into SG (B x D, contiguous);
 *   records    : per-sample scalars of gsm_numpy.py:8-17 from the gathered SG -> records as above (replicated);
 *   apply rows : Srows = S0rows + (1/B) sum_b (d_b d_b^T - e_b e_b^T)[row0 : row0+nrows, :], and the full new
 *                mean when mu != NULL.
 */
int gsmvi_gsm_rows_stage_f64(gsmvi_ctx* ctx, void* stream, int D, int B, int nrows,
                             const double* G, int ldg, const double* S0rows, int lds0,
                             double* SGcols, int ldsg);
int gsmvi_gsm_records_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                          const double* X, int ldx, const double* G, int ldg, const double* mu0,
                          const double* SG, double* rec, int ldrec);
int gsmvi_gsm_apply_rows_f64(gsmvi_ctx* ctx, void* stream, int D, int B, int row0, int nrows,
                             const double* rec, int ldrec, const double* mu0,
                             const double* S0rows, int lds0, double* mu, double* Srows, int lds);

/*
 * Factor-form GSM update (BASELINE config 5): the state is a square factor Fm with
 * Sigma = Fm^T Fm; Z (B x D) are the whitened draws behind the samples X = 1 mu0^T + Z F0, G = lp_g(X).
 * Produces (mu, F) with F^T F equal to the covariance gsm_numpy.gsm_update would return for
 * (X, G, mu0, F0^T F0) -- without forming or factorising any D x D covariance: the positive-definite
 * test of gsm_numpy.py:121-125,132-146 becomes a Cholesky of a 2B x 2B matrix.  If that test fails,
 * (mu, F) = (mu0, F0) and *info_dev = 1 (revert); else *info_dev = 0.  Needs 2B <= D and 2B <= 256 (2B <= 64: the chain is one workgroup; <= 128: one-workgroup
 * factorisations; <= 256: two-level blocked, round 4).
 * n_reverts_dev (device int, may be NULL) is incremented on a revert, like gsmvi_commit_f64 does.
 */
int gsmvi_gsm_factor_update_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                                const double* Z, int ldz, const double* X, int ldx, const double* G, int ldg,
                                const double* mu0, const double* F0, int ldf0,
                                double* mu, double* F, int ldf, int* info_dev, int* n_reverts_dev);

/*
 * The factor-form update in two stages, for the batch-sharded multi-GPU path (BASELINE config 5 on several GPUs;
 * same decomposition as gsmvi_gsm_local_stage_f64 / gsmvi_gsm_apply_f64):
 *   local stage : for this rank's B_local samples (rows of Z, X, G): W = G F0^T, the whitened residual v_b = w_b + z_b
 *                 and v_b F0; one record per sample  rec[b] = [ x_b - mu0 (D) | v_b (D) | v_b F0 (D) ], row stride
 *                 ldrec >= gsmvi_gsm_record_len(D).  Two of the three passes over F0 are divided by the number of
 *                 ranks.  Records of all ranks are all-gathered (RCCL) by the caller;
 *   apply       : every replica holds the same Z (B x D: the draw stream is replicated, gsmvi_randn_f64 is
 *                 counter-based) and all B records, and runs the Gram product of [Z; V], the per-sample scalars (they are
 *                 entries of that Gram matrix), the 2B x 2B positive-definite test and the rank-2B factor update.  Same outputs and revert semantics as gsmvi_gsm_factor_update_f64.
 * gsmvi_gsm_factor_update_f64 == local stage with B_local = B followed by apply.
 */
int gsmvi_gsm_factor_local_stage_f64(gsmvi_ctx* ctx, void* stream, int D, int B_local,
                                     const double* Z, int ldz, const double* X, int ldx, const double* G, int ldg,
                                     const double* mu0, const double* F0, int ldf0, double* rec, int ldrec);
int gsmvi_gsm_factor_apply_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                               const double* Z, int ldz, const double* rec, int ldrec,
                               const double* mu0, const double* F0, int ldf0,
                               double* mu, double* F, int ldf, int* info_dev, int* n_reverts_dev);

/*
 * The factor-form update batch-sharded over RCCL in ONE call: local stage on this rank's rows -> ncclAllGather of the
 * records (in place in rec_all: (B_local * nranks) x gsmvi_gsm_record_len(D) doubles) -> combined update on every replica.
 * Z_all holds the replicated draws of ALL B = B_local * nranks samples (the draw stream is counter-based; rank r's samples
 * are rows [r B_local, (r + 1) B_local)); X_local, G_local are this rank's rows.  Same outputs and revert semantics as
 * gsmvi_gsm_factor_update_f64; everything is validated before the first launch.
 */
int gsmvi_gsm_factor_update_sharded_f64(gsmvi_ctx* ctx, void* stream, void* nccl_comm, int D, int B_local,
                                        const double* Z_all, int ldz, const double* X_local, int ldx,
                                        const double* G_local, int ldg, const double* mu0, const double* F0, int ldf0,
                                        double* rec_all, double* mu, double* F, int ldf, int* info_dev,
                                        int* n_reverts_dev);

/*
 * Profiling mode (used by bench.py for the roofline line): when on, the three kernels of the GSM
 * update are launched with dispatch-timestamp events; gsmvi_get_profile waits for the last call
 * and returns the kernel durations in milliseconds: ms[0] panel product, ms[1] per-sample
 * scalars, ms[2] covariance update.  A slot is -1 when that launch did not run in the last profiled call: the two-launch
 * form of the update (GSMVI_PATH_GSM_TWO_LAUNCH) has no per-sample launch, so ms[1] = -1 there -- never a stale time.
 */
int gsmvi_set_profiling(gsmvi_ctx* ctx, int on);
int gsmvi_get_profile(gsmvi_ctx* ctx, float* ms, int n);

/*
 * Which kernel families the calls on this context launched since the last reset (round 5).  The tuned kernels need
 * D % 64 == 0, even leading dimensions and 16-byte aligned bases (any batch size); everything else runs the guarded
 * kernels of the same arithmetic (csrc/gsmvi_kernels.hip), about half as fast.  The reference takes any (D, B)
 * (gsm_numpy.py:27-55, bam.py:31-114); a caller that keeps its state padded to a multiple of 64 columns (zero border in
 * mu, X, G, Z, F; identity border on the diagonal of Sigma -- INTEGRATION.md, "Off-grid dimensions") stays on the tuned
 * kernels for every D, and this query is how tests and profiles prove that it did: *bits & GSMVI_PATH_GENERIC_MASK == 0.
 * reset != 0 clears the record after reading it.
 */
#define GSMVI_PATH_PANEL_FAST 0x0001u      /* k_panel_fast: A M products (S0 G, score, sampler, V Fm, ...)          */
#define GSMVI_PATH_PANEL_WIDE 0x0002u      /* k_panel_wide: the same on 64 x 64 tiles (64-row panels, D >= 1024)    */
#define GSMVI_PATH_PANEL_GENERIC 0x0004u   /* k_panel_partial                                                       */
#define GSMVI_PATH_PANEL_T_FAST 0x0008u    /* k_panel_t_fast: A M^T products (W = G F^T, Gram matrices)              */
#define GSMVI_PATH_PANEL_T_GENERIC 0x0010u /* k_panel_t                                                             */
#define GSMVI_PATH_SCALARS_FAST 0x0020u    /* k_gsm_scalars_fast                                                    */
#define GSMVI_PATH_SCALARS_GENERIC 0x0040u /* k_gsm_scalars                                                         */
#define GSMVI_PATH_COV_SYM 0x0080u         /* k_gsm_cov_sym / k_gsm_cov_sym_p: the headline covariance kernel       */
#define GSMVI_PATH_COV_GENERIC 0x0100u     /* k_gsm_cov_update (also: non-symmetric S0, row-block shards)           */
#define GSMVI_PATH_FUPD_FAST 0x0200u       /* k_gsmf_update_fs / k_gsmf_update_fast: F = F0 + Rt^T Fs               */
#define GSMVI_PATH_FUPD_GENERIC 0x0400u    /* k_gsmf_update + k_gsmf_mean                                           */
#define GSMVI_PATH_LOWRANK_FAST 0x0800u    /* k_lowrank_update_fast: BaM's S = S0 + Vf^T Vf - Z^T Z                 */
#define GSMVI_PATH_LOWRANK_GENERIC 0x1000u /* k_lowrank_update                                                      */
#define GSMVI_PATH_BATCHED 0x2000u         /* k_gsm_batched / k_gauss_score_batched: the batched entry points      */
#define GSMVI_PATH_BATCHED_BAM 0x4000u     /* k_bam_batched: the batched BaM entry points                           */
#define GSMVI_PATH_BATCHED_KL 0x8000u      /* k_kl_batched: the batched KL monitor's entry points                  */
#define GSMVI_PATH_BATCHED_ADVI 0x10000u   /* k_advi_batched / k_advi_cov_batched: the batched ADVI entry points   */
#define GSMVI_PATH_BATCHED_TARGET 0x20000u /* k_logistic_batched: the batched non-Gaussian target's entry point; with GSMVI_PATH_BATCHED_LAPLACE in one call: k_laplace_shared_batched, k_negbin_laplace_batched or k_ordinal_laplace_batched; with GSMVI_PATH_BATCHED_LOO in one call: k_psis_loo_negbin_batched or k_psis_loo_ordinal_batched; with GSMVI_PATH_BATCHED_PREDICT in one call: k_negbin_predict_batched, k_ordinal_predict_batched or k_glm_shared_predict_batched (all 32 bits are taken; no other call sets any of these pairs) */
#define GSMVI_PATH_BATCHED_LBFGS 0x40000u  /* k_lbfgs_step_batched / k_lbfgs_hess_inv_batched: the batched initialiser   */
#define GSMVI_PATH_BATCHED_LAPLACE 0x80000u /* k_laplace_batched: the batched GLM Hessian and Newton step; with GSMVI_PATH_BATCHED_TARGET in one call: k_laplace_shared_batched, the shared-design Hessian and Newton step, k_negbin_laplace_batched, the negative binomial one, or k_ordinal_laplace_batched, the ordinal one */
#define GSMVI_PATH_BATCHED_PREDICT 0x100000u /* k_glm_predict_batched: the batched GLM posterior predictive; with GSMVI_PATH_BATCHED_SOFTMAX: k_softmax_predict_batched; with GSMVI_PATH_BATCHED_TARGET: k_negbin_predict_batched, k_ordinal_predict_batched, the ordinal predictive, or k_glm_shared_predict_batched, the shared-design GLM predictive */
#define GSMVI_PATH_BATCHED_PSIS 0x200000u /* k_psis_batched: the batched Pareto-smoothed importance diagnostic            */
#define GSMVI_PATH_BATCHED_LOO 0x400000u /* k_psis_loo_batched: the batched PSIS leave-one-out; with GSMVI_PATH_BATCHED_SOFTMAX: k_psis_loo_softmax_batched; with GSMVI_PATH_BATCHED_TARGET: k_psis_loo_negbin_batched or k_psis_loo_ordinal_batched */
#define GSMVI_PATH_GSM_TWO_LAUNCH 0x800000u /* the dense GSM update ran as two launches (no k_gsm_scalars_fast, no records)          */
#define GSMVI_PATH_BATCHED_SOFTMAX 0x1000000u /* k_softmax_batched: the batched multinomial logit target's entry point            */
#define GSMVI_PATH_PANEL_CHUNK512 0x2000000u /* the two-launch product ran as two slabs of one 512-row chunk each (D = 1024, no explicit "panel_kc") */
#define GSMVI_PATH_BATCHED_PATHFINDER 0x4000000u /* k_pf_propose / k_pf_select: the batched Pathfinder initialiser                  */
#define GSMVI_PATH_COV_FOLD_DIAG 0x8000000u /* the two-launch covariance launch ran without single-tile workgroups: diagonal leftovers folded ("cov_fold_diag") */
#define GSMVI_PATH_BATCHED_SOFTMAX_LAPLACE 0x10000000u /* k_softmax_laplace_batched: the batched multinomial logit Hessian and Newton step */
#define GSMVI_PATH_COV_S0_LAST 0x20000000u /* the two-slab covariance launch issued and waited for its S0 tile last ("cov_s0_last") */
#define GSMVI_PATH_COV_STORE_WT 0x40000000u /* the two-slab covariance launch stored S write-through ("cov_store_wt") */
#define GSMVI_PATH_PANEL_QM_WHOLE 0x80000000u /* the two-slab product left one Qm value per sample ("panel_qm_whole") */
#define GSMVI_PATH_GENERIC_MASK (0x0004u | 0x0010u | 0x0040u | 0x0100u | 0x0400u | 0x1000u)
int gsmvi_last_path(gsmvi_ctx* ctx, unsigned* bits, int reset);

/*
 * Where the BaM entry points of this context take the regulariser from (round 5).  The reference evaluates regf(i) on the
 * host in every iteration (bam.py:196) and passes a number; a caller that captures an iteration into a hipGraph needs a
 * value that can change between replays.  reg_dev != NULL: every BaM update launched on this context from now on (dense,
 * factor form, and the sharded forms built on them) reads *reg_dev on the DEVICE when its kernels execute and ignores its `reg`
 * argument (which is still validated: pass any positive number; the value in the word is the caller's to check, reg > 0); the word
 * must stay valid while such work is pending.  NULL (the default) restores the by-value argument.
 */
int gsmvi_bam_set_reg_source(gsmvi_ctx* ctx, const double* reg_dev);

/*
 * Score of the Gaussian target N(m, P^-1) at the rows of X: G = -(X - 1 m^T) P.
 * Replaces the user callback of examples/example_gsm_numpy.py:24-29 (P symmetric precision matrix).
 */
int gsmvi_gaussian_score_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                             const double* X, int ldx, const double* m,
                             const double* P, int ldp, double* G, int ldg);

/*
 * Batched GSM (K independent problems of the same (D, B)): 1 <= D <= 64, 1 <= B <= 32, K >= 1 (one launch each: K < 2^24 for
 * D > 16, K < 2^26 for D <= 16).  Every array is packed and contiguous with a leading problem axis -- X, G (K x B x D),
 * mu (K x D), S, R (K x D x D) -- in device memory; problem k reads and writes only slice k of each, so a NaN or a revert in
 * one problem cannot reach another.  Shapes, NULL arrays and overlaps are checked before the context is looked at (then a
 * NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  The overlap rule of every batched entry
 * point: an array that a kernel may write (an output, a fit's state or counters, a fit step's X) must not overlap any other
 * array of the call, NULL ones aside; read-only arrays may overlap each other.  No context workspace is used (the kernels
 * keep a problem in LDS).  Sets GSMVI_PATH_BATCHED.
 *
 * gsmvi/gsm_numpy.py:27-55 gsm_update under jax.vmap (gsmvi/gsm.py:31-58) -> gsmvi_gsm_update_batched_f64:
 *   (mu_k, S_k) = gsm_update(X_k, G_k, mu0_k, S0_k) for every k.  Reads ALL of S0_k (both triangles: the reference's literal
 *   S0 + mean semantics for any square S0); S_k is exactly symmetric when S0_k is.  Outputs must not overlap inputs.
 */
int gsmvi_gsm_update_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* G,
                                 const double* mu0, const double* S0, double* mu, double* S);

/*
 * The start of a batched dense fit (gsmvi/gsm_numpy.py:103-116 per problem): R_k = upper Cholesky factor of cov_k (reads all of
 * cov_k; the factorisation uses its upper triangle) and info_dev[k] = 0, or 1 + the first bad pivot (not > 0, NaN, inf).
 * seeds_dev (K uint64 keys, may be NULL): X_k = mean_k + Z_k R_k with Z_k = draw 0 of key seeds_dev[k] of the stream of
 * gsmvi_randn_f64, laid out as B x (D + 1) normals with the last column dropped for odd D (the layout of the single fit).
 */
int gsmvi_gsm_fit_init_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* mean, const double* cov,
                                   double* R, int* info_dev, const uint64_t* seeds_dev, double* X);

/*
 * One iteration of the batched dense fit after the score G = lp_g(X) (gsmvi/gsm_numpy.py:116-125 per problem), one launch:
 * the update of every problem, the Cholesky test of its new covariance (_check_goodness, gsm_numpy.py:132-146), and per
 * problem: accept -> (mean_k, cov_k, R_k) <- (mu', S', chol(S')); revert -> all three kept bit for bit, n_reverts_dev[k] += 1
 * (may be NULL).  info_dev (may be NULL) receives each problem's test result as gsmvi_gsm_fit_init_batched_f64 defines it.
 * seeds_dev != NULL: X is overwritten with the next samples, X_k = mean_k + Z_k R_k of the (kept or accepted) state with Z_k =
 * draw `call` of key seeds_dev[k] (needs R).  seeds_dev == NULL: X is left alone (teacher-forced samples; R may be NULL).
 */
int gsmvi_gsm_fit_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, double* X, const double* G, double* mean,
                                   double* cov, double* R, int* info_dev, int* n_reverts_dev, const uint64_t* seeds_dev,
                                   uint64_t call);

/*
 * examples/example_gsm_numpy.py:24-29 for K Gaussian targets -> gsmvi_gaussian_score_batched_f64: G_k = -(X_k - 1 m_k^T) P_k
 * (m: K x D, P: K x D x D symmetric precision matrices).  G must not overlap an input; K B D < 2^32 - 256.
 */
int gsmvi_gaussian_score_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* m,
                                     const double* P, double* G);

/*
 * Batched BaM (K independent problems of the same (D, B)), with the bounds, the layout and the per-problem isolation of the
 * batched GSM above: 1 <= D <= 64, 1 <= B <= 32 (B > D is legal), K >= 1 (K < 2^24 when a problem takes a whole workgroup,
 * K < 2^26 when four share one: D <= 16 and four problems' LDS within 160 KiB).  X, G (K x B x D), mu (K x D), S, R (K x D x D),
 * packed, in device memory.  reg_dev: NULL = the scalar `reg` for every problem, else K per-problem values on the device.
 * Shapes, NULL arrays and overlaps are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  No context workspace is used.  Sets GSMVI_PATH_BATCHED_BAM.
 *
 * gsmvi/bam.py:72-114 bam_lowrank_update (= bam.py:31-69, K6) under jax.vmap -> gsmvi_bam_update_batched_f64:
 *   (mu_k, S_k) = bam_update(X_k, G_k, mu0_k, S0_k, reg_k) with the exact rank-B factor of U (as gsmvi_bam_update_f64), S_k
 *   symmetrised and jitter added to its diagonal (bam.py:198-199; jitter = 0 for the update alone).  info_dev (may be NULL):
 *   0, or 1 when problem k's B x B chain failed (non-finite input, or BB not positive definite); its mu_k and S_k are NaN.
 *   Outputs must not overlap inputs.
 */
int gsmvi_bam_update_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* G,
                                 const double* mu0, const double* S0, double reg, const double* reg_dev, double jitter,
                                 double* mu, double* S, int* info_dev);

/*
 * One iteration of the batched BaM fit after the score G = lp_g(X) (gsmvi/bam.py:189-212 per problem), one launch: the update
 * of every problem (as gsmvi_bam_update_batched_f64), + jitter I, symmetrised (:198-199), the Cholesky test of the new
 * covariance (:208), and per problem: accept -> (mean_k, cov_k, R_k) <- (mu', S', chol(S')); revert -> all three kept bit for
 * bit, n_reverts_dev[k] += 1 (may be NULL).  A failed chain or a non-finite score reverts its problem.  info_dev (may be NULL):
 * 0, or 1 + the first bad pivot of the test.  The fit starts with gsmvi_gsm_fit_init_batched_f64 (chol of the initial cov, draw 0).
 * seeds_dev != NULL: Xout (may equal X, must not overlap anything else) receives the next samples, Xout_k = mean_k + Z_k R_k of
 * the kept or accepted state, Z_k = draw `call` of key seeds_dev[k] (B x (D + 1) normals, column D dropped, for odd D; needs
 * R).  seeds_dev == NULL: nothing is drawn (teacher-forced samples; R and Xout may be NULL).  info_dev and n_reverts_dev
 * must not overlap each other or any double array; no output may overlap G, seeds_dev or reg_dev.
 */
int gsmvi_bam_fit_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* X, const double* G,
                                   double* mean, double* cov, double* R, double reg, const double* reg_dev, double jitter,
                                   int* info_dev, int* n_reverts_dev, const uint64_t* seeds_dev, uint64_t call, double* Xout);

/*
 * Batched KL monitor (K Gaussians q_k = N(mean_k, cov_k) of one D): 1 <= D <= 64, K >= 1 with the grid limits of the batched GSM
 * above, nc >= 1 rows per call.  mean (K x D), cov (K x D x D), X, Y (K x nc x D), logq_sum (K), info (K), packed, in device
 * memory.  Both factor cov_k = R_k^T R_k (upper, in LDS: only the upper triangle of cov_k is used) and write info[k] = 0, or
 * 1 + the first pivot that is not > 0 and finite; such a problem gets logq_sum[k] = NaN (and NaN rows of X) and no other
 * problem is touched.  mean and cov are only read and no context workspace is used, so a call may sit between two steps of a
 * running batched fit.  Shapes, NULL arrays and overlaps are checked before the context is looked at (then a NULL ctx); every
 * failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Sets GSMVI_PATH_BATCHED_KL.
 *
 * gsmvi/monitors.py:83-125, the reverse-KL samples of KLMonitor.__call__ (:101-103) and MultivariateNormal.log_prob on them
 * (:104-113), for every k -> gsmvi_kl_draw_batched_f64: the rows s = s0 .. s0 + nc - 1 of draw `call` of key seeds[k],
 *   z_s = elements s D .. s D + D - 1 of gsmvi_randn_f64(seeds[k], call, n D) (the plain layout: pair (s D + j) / 2, no odd-D
 *   padding), X_k row s - s0 = mean_k + z_s R_k, and logq_sum[k] = sum_s (-|z_s|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi).
 *   A call split into chunks (s0 > 0) writes the same X rows, bit for bit, as the unsplit call.
 */
int gsmvi_kl_draw_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t nc, int64_t s0, const double* mean,
                              const double* cov, const uint64_t* seeds, uint64_t call, double* X, double* logq_sum, int* info);

/*
 * gsmvi/monitors.py:104-113 MultivariateNormal(mean_k, cov_k).log_prob on the rows of Y_k (the forward-KL reference samples,
 * :110-113), for every k -> gsmvi_logq_batched_f64: w = the solution of R_k^T w = y - mean_k (forward substitution) and
 * logq_sum[k] = sum over the nc rows of (-|w|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi).
 */
int gsmvi_logq_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t nc, const double* mean, const double* cov,
                           const double* Y, double* logq_sum, int* info);

/*
 * Batched ADVI (K independent full-rank fits of the same (D, B); the ELBO baseline of gsmvi/advi.py), with the bounds, the
 * layout and the per-problem isolation of the batched GSM above: 1 <= D <= 64, 1 <= B <= 32, K >= 1.  The family is
 * N(loc_k, L_k L_k^T), L_k lower triangular; `scales` (K x D (D + 1) / 2, packed) holds the entries of L_k in np.tril_indices
 * order (row-major over the lower triangle: entry (i, j), j <= i, at i (i + 1) / 2 + j; advi.py:23-27,80-83).  loc, m_loc, v_loc
 * (K x D), scales, m_s, v_s (K x D (D + 1) / 2), G, X, Z (K x B x D), logq_sum, lr_dev (K), packed, in device memory.  Draws:
 * draw c of key seeds_dev[k] is B x (D + 1) normals for odd D, column D dropped -- the layout of the batched GSM and BaM fits,
 * so the same keys give the same z to all three.  Shapes, NULL arrays and overlaps are checked before the context is looked at
 * (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  No context workspace is used.  Sets
 * GSMVI_PATH_BATCHED_ADVI.
 *
 * gsmvi/advi.py:80-86, the start of a fit -> gsmvi_advi_init_batched_f64: scales_k = the lower Cholesky factor of cov_k (the
 *   factorisation reads the upper triangle of cov_k), info_dev[k] as gsmvi_gsm_fit_init_batched_f64 defines it.  With seeds_dev
 *   (z = draw 0) or Z (K x B x D given normals; not both): X_k = loc_k + Z_k L_k^T and
 *   logq_sum[k] = sum_b (-|z_b|^2 / 2) - B sum_i log|L_ii| - B D / 2 log 2 pi; with neither, X and logq_sum must be NULL.
 */
int gsmvi_advi_init_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* mean, const double* cov,
                                double* scales, int* info_dev, const uint64_t* seeds_dev, const double* Z, double* X,
                                double* logq_sum);

/*
 * gsmvi/advi.py:31-45 (the loss and its gradient) and :69-73 (the optimiser step), one iteration after the score G = lp_g(X),
 * one launch -> gsmvi_advi_step_batched_f64.  With z the normals behind X (x_b = loc + L z_b), the gradient of the loss
 * -(sum_b lp(x_b) - sum_b log q(x_b)) is  d / d loc = -sum_b g_b,  d / d L_ij = -sum_b g_bi z_bj (j <= i), and -B / L_ii more on
 * the diagonal.  Adam, in place on loc, scales and the moments: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2,
 * p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps), t = iteration + 1 >= 1 (torch.optim.Adam at its defaults,
 * optax.adam).  lr_dev: NULL = the scalar lr for every problem, else K per-problem values.  Then, unless Xout is NULL, the next
 * samples Xout_k = loc_k + Z_k L_k^T and their logq_sum[k] (as in the init) from the UPDATED state; Xout and logq_sum go together.
 * seeds_dev != NULL: the z behind G is draw call - 1 of key seeds_dev[k] (call >= 1), regenerated in the kernel, and the next z is
 * draw call; Zcur and Znext must be NULL.  seeds_dev == NULL: Zcur (K x B x D) is the z behind G and, with Xout, Znext the next z.
 * A non-finite score is not caught: it makes that problem's state NaN from then on, and touches no other problem.
 * Written: loc, scales, the moments, Xout, logq_sum; none of them may overlap any other array of the call.
 */
int gsmvi_advi_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int B, const double* G, double* loc,
                                double* scales, double* m_loc, double* v_loc, double* m_s, double* v_s, int64_t t, double lr,
                                const double* lr_dev, double b1, double b2, double eps, const uint64_t* seeds_dev, uint64_t call,
                                const double* Zcur, const double* Znext, double* Xout, double* logq_sum);

/*
 * gsmvi/advi.py:23-27 scales_to_cov for K problems -> gsmvi_advi_cov_batched_f64: cov_k = L_k L_k^T (K x D x D), exactly
 * symmetric (entries (i, j) and (j, i) sum the same products in the same order).
 */
int gsmvi_advi_cov_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, const double* scales, double* cov);

/*
 * Batched logistic target: the log-density and the score of K Bayesian logistic regressions of one (N, D) at nc points each,
 * one launch.  examples/example_gsm.py:34-35, the model's log_prob and lp_g = jit(grad(...)) of it (which XLA fuses into a
 * kernel or two), for this model -> gsmvi_logistic_batched_f64.  Problem k has the design matrix A_k (N rows a_n of length D),
 * labels y_kn in [0, 1] (soft labels allowed), n_k valid rows and prior precision lam_k >= 0 (prior N(0, I / lam_k); 0 = flat).
 * At the rows x of X_k, with eta_n = a_n . x:
 *   lp[k, c] = sum_{n < n_k} [ y_n eta_n - softplus(eta_n) ] - lam_k |x|^2 / 2         (unnormalised log posterior)
 *   G[k, c]  = sum_{n < n_k} ( y_n - sigma(eta_n) ) a_n - lam_k x
 * in the overflow-safe forms e = exp(-|eta|), sigma = 1 / (1 + e) for eta >= 0 and e / (1 + e) otherwise, softplus =
 * max(eta, 0) + log1p(e).  A (K x N x D), y (K x N), X, G (K x nc x D), lp (K x nc), packed, in device memory; 1 <= D <= 64 and K
 * with the grid limits of the batched GSM above; nc >= 1 and N >= 1 are not bounded by LDS (both are walked in tiles).
 * counts_dev: NULL = N valid rows everywhere, else K ints on the device, each clamped to 0 .. N in the kernel (the host does not
 * read them); rows n >= n_k are never loaded, whatever they hold.  prior_prec_dev: NULL = the scalar prior_prec for every
 * problem, else K values.  At least one of G, lp is given; G alone evaluates no logarithm.  Every output row sums over n in the
 * order 0 .. n_k - 1 and depends on A_k, y_k, n_k, lam_k and its own row of X only: the same bits for any K, nc and neighbours.
 * A row of X with a non-finite entry gets NaN outputs and no other row is touched; a non-finite entry in a valid row of A_k or
 * y_k stays in problem k.  Shapes, NULL arrays and overlaps (G and lp are the written arrays) are checked before the context is
 * looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no
 * context workspace is used.  Sets GSMVI_PATH_BATCHED_TARGET.
 */
int gsmvi_logistic_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int nc, int64_t N, const double* A, const double* y,
                               const int* counts_dev, double prior_prec, const double* prior_prec_dev, const double* X, double* G,
                               double* lp);

/*
 * Batched GLM targets: the same launch for a family of generalised linear models.  examples/example_gsm.py:34-35, a model's
 * log_prob and lp_g = jit(grad(...)) of it, for K Poisson, probit, Gaussian or logistic regressions of one (N, D) ->
 * gsmvi_glm_batched_f64.  Everything is as in gsmvi_logistic_batched_f64 above except the link and the offset: with
 * eta_n = a_n . x + o_kn (offset (K x N) on the device, NULL = no offset),
 *   lp[k, c] = sum_{n < n_k} t(eta_n, y_n) - lam_k |x|^2 / 2,      G[k, c] = sum_{n < n_k} r(eta_n, y_n) a_n - lam_k x,
 *   family                 y                    r = dt / d eta                               t
 *   GSMVI_GLM_LOGISTIC     in [0, 1]            y - sigma(eta)                               y eta - softplus(eta)
 *   GSMVI_GLM_POISSON      >= 0, finite         y - e^eta                                    y eta - e^eta   (log link; -log y! dropped)
 *   GSMVI_GLM_PROBIT       in [0, 1]            y phi/Phi(eta) - (1 - y) phi/Phi(-eta)       y log Phi(eta) + (1 - y) log Phi(-eta)
 *   GSMVI_GLM_GAUSSIAN     finite               tau_k (y - eta)                              -tau_k (y - eta)^2 / 2   (identity link)
 * The probit link is evaluated from u = erfcx(|eta| / sqrt 2) and e = exp(-eta^2 / 2): log Phi(-|eta|) = log(u / 2) - eta^2 / 2,
 * phi / Phi(-|eta|) = sqrt(2 / pi) / u, log Phi(|eta|) = log1p(-u e / 2), phi / Phi(|eta|) = e / sqrt(2 pi) / (1 - u e / 2): finite out
 * to |eta| = 1e4.  The ranges of y are the caller's to keep (not checked here).  noise_prec / noise_prec_dev (NULL = the scalar,
 * else K values tau_k on the device) belong to the Gaussian family, where the scalar must be finite and > 0; for any other
 * family anything but 1.0 and NULL is GSMVI_ERR_BAD_ARG, as is an unknown family.  GSMVI_GLM_LOGISTIC with offset = NULL gives the
 * bits of gsmvi_logistic_batched_f64.  The rules of that entry point hold: rows n >= n_k are never loaded, every output row sums
 * n = 0 .. n_k - 1 in order in one thread (the same bits for any K, nc and neighbours), a row of X with a non-finite entry gets NaN
 * outputs.  Poisson adds: a row of X for which some valid e^eta is not finite (eta above 709.78) gets NaN outputs in the same way,
 * and no other row or problem is touched.  Checks (offset and noise_prec_dev are read-only arrays of the overlap rule) come
 * before the context is looked at; inputs are only read; no context workspace.  Sets GSMVI_PATH_BATCHED_TARGET.
 */
#define GSMVI_GLM_LOGISTIC 0
#define GSMVI_GLM_POISSON 1
#define GSMVI_GLM_PROBIT 2
#define GSMVI_GLM_GAUSSIAN 3
int gsmvi_glm_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int nc, int64_t N, int family, const double* A,
                          const double* y, const double* offset, const int* counts_dev, double noise_prec,
                          const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, const double* X, double* G,
                          double* lp);

/*
 * Shared-design GLM target: the same four families for K problems that share ONE design matrix.  examples/example_gsm.py:34-35, a
 * model's log_prob and lp_g = jit(grad(...)) of it, for K regressions on the same covariates (many responses, a sweep over the
 * precisions, the Bayesian bootstrap) -> gsmvi_glm_shared_batched_f64.  A is (N x D), shared; y, offset (NULL = none) and weights
 * (NULL = 1 everywhere) are (K x N) on the device; X, G (K x nc x D), lp (K x nc).  With eta_n = a_n . x + o_kn and (r, t) the
 * family's link of gsmvi_glm_batched_f64 above,
 *   lp[k, c] = sum_n w_kn t(eta_n, y_kn) - lam_k |x|^2 / 2,      G[k, c] = sum_n w_kn r(eta_n, y_kn) a_n - lam_k x.
 * The K nc rows of X are stacked into one tall matrix and both sums run on the f64 MFMA against tiles of A: no copy of A per
 * problem.  1 <= D <= 64, any N >= 1 and nc >= 1, K with the grid limits of gsmvi_glm_batched_f64 and K nc <= 64 (2^31 - 1).  There
 * is no counts argument: a weight of 0 says the same.  An observation with w_kn = 0 (or a weight that is not > 0) contributes
 * exactly nothing whatever y_kn, o_kn and eta hold there (removed by selection, not multiplied by 0); the weights' sign and the
 * ranges of y are the caller's to keep.  The precisions are as in gsmvi_glm_batched_f64 (noise_prec: the Gaussian family only).
 * Every output row sums over n in an order fixed by N alone (G: one accumulation chain over n ascending; lp: four interleaved
 * partial sums added in a fixed order), with no atomics: the same bits from run to run, for any K and nc, alone or among other
 * rows and problems.  A row of X with a non-finite entry gets NaN outputs, and a Poisson row for which some e^eta at an
 * observation with w > 0 is not finite does; no other row is touched.  A non-finite entry of A reaches every problem (A is
 * shared).  Checks (shapes, family, precisions, NULL arrays, G or lp, overlaps: G and lp are the written arrays, every other
 * array is read-only) come before the context is looked at (then a NULL ctx) and return GSMVI_ERR_BAD_ARG before anything is
 * enqueued.  Inputs are only read; no context workspace.  Sets GSMVI_PATH_BATCHED_TARGET.
 */
int gsmvi_glm_shared_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int nc, int64_t N, int family, const double* A,
                                 const double* y, const double* offset, const double* weights, double noise_prec,
                                 const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, const double* X,
                                 double* G, double* lp);

/*
 * Batched negative binomial target: the log-density and the score of K overdispersed count regressions of one (N, P) at nc points
 * each, one launch.  examples/example_gsm.py:34-35, a model's log_prob and lp_g = jit(grad(...)) of it, for counts whose variance
 * exceeds their mean -> gsmvi_negbin_batched_f64.  Problem k has the design matrix A_k (N rows a_n of P columns), responses
 * y_kn >= 0 (finite; they need not be integers), an optional offset o_kn (NULL = none), n_k valid rows, and the parameter
 * x = (beta, theta) of length D = P + 1: theta = log r is the log of the size (variance mu + mu^2 / r; r -> inf is Poisson).  With
 * eta_n = a_n . beta + o_n, d_n = eta_n - theta, r = e^theta, dlg(y, r) = lgamma(y + r) - lgamma(r), dps(y, r) = psi(y + r) - psi(r):
 *   t       = dlg(y, r) - r softplus(d) - y softplus(-d)        (log NB(y | mu = e^eta, r) without -lgamma(y + 1))
 *   r_eta   = y sigma(-d) - r sigma(d)                          (= dt / d eta)
 *   r_theta = r (dps(y, r) - softplus(d)) - r_eta               (= dt / d theta)
 *   lp[k, c]      = sum_{n < n_k} t_n - lam_k |beta|^2 / 2 - kap_k (theta - m_k)^2 / 2
 *   G[k, c, :P]   = sum_{n < n_k} r_eta,n a_n - lam_k beta
 *   G[k, c, P]    = sum_{n < n_k} r_theta,n - kap_k (theta - m_k)
 * The two differences are evaluated as differences of Stirling's series (after ten steps of the recurrence for r < 10), never as
 * two calls: accurate to a few eps of the terms of t, r_eta and r_theta as written.  e^eta is never formed, so there is no overflow
 * rule as for the Poisson family: the outputs are finite wherever the truth is.  A (K x N x P), y, offset (K x N), X, G
 * (K x nc x (P + 1)), lp (K x nc), packed, in device memory; 1 <= P <= 63; K, nc, N, counts_dev and prior_prec / prior_prec_dev
 * (lam, the prior N(0, I / lam_k) of beta) as in gsmvi_glm_batched_f64; theta_mean / theta_mean_dev (m, finite) and theta_prec /
 * theta_prec_dev (kap, finite and >= 0; 0 = flat) in the same scalar-or-K-values style: the prior N(m_k, 1 / kap_k) of theta.
 * At least one of G, lp is given.  Every output row sums over n in the order 0 .. n_k - 1 in one thread (r_theta into the last
 * component) and depends on its problem and its own row of X only: the same bits for any K, nc and neighbours; no atomics.  Rows
 * n >= n_k are never loaded; n_k = 0 leaves the two priors.  A row of X with a non-finite entry, or whose e^theta is not a positive
 * normal number (|theta| above 708), gets NaN outputs and no other row is touched.  Shapes, priors, NULL arrays and overlaps (G and
 * lp are the written arrays) are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace.  Sets GSMVI_PATH_BATCHED_TARGET.
 */
int gsmvi_negbin_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int nc, int64_t N, const double* A, const double* y,
                             const double* offset, const int* counts_dev, double theta_mean, const double* theta_mean_dev,
                             double theta_prec, const double* theta_prec_dev, double prior_prec, const double* prior_prec_dev,
                             const double* X, double* G, double* lp);

/*
 * Batched ordinal target: the log-density and the score of K cumulative-logit (proportional odds) regressions of one (N, P, C) at nc
 * points each, one launch.  examples/example_gsm.py:34-35, a model's log_prob and lp_g = jit(grad(...)) of it, for an ordered
 * response (ratings, grades, severity scores) -> gsmvi_ordinal_batched_f64.  Problem k has the design matrix A_k (N rows a_n of P
 * columns, no intercept column), integer labels y_kn in 0 .. C - 1, an optional offset o_kn (NULL = none), n_k valid rows, and the
 * parameter x = (beta, delta) of length D = P + C - 1.  The cutpoints are ordered by construction:
 *   cut_0 = delta_0,   cut_j = cut_{j-1} + e^{delta_j}   (j = 1 .. C - 2)
 * and P(y_n = c) = sigma(cut_c - eta_n) - sigma(cut_{c-1} - eta_n) with eta_n = a_n . beta + o_n, cut_{-1} = -inf, cut_{C-1} = +inf.
 * With a = cut_{y-1} - eta (y >= 1), b = cut_y - eta (y <= C - 2) and, for an interior class 1 <= y <= C - 2, w = e^{delta_y}:
 *   t     = -[y <= C-2] softplus(-b) - [y >= 1] softplus(a) + [interior] log(1 - e^{-w})
 *   u_lo  = -sigma(a) - [interior] / expm1(w)     (= dt / d cut_{y-1}; y >= 1, else 0)
 *   u_hi  = sigma(-b) + [interior] / expm1(w)     (= dt / d cut_y;     y <= C-2, else 0)
 *   r_eta = sigma(a) - sigma(-b)                  (= dt / d eta)
 *   lp[k, c]       = sum_{n < n_k} t_n - lam_k |beta|^2 / 2 - kap_k |delta|^2 / 2
 *   G[k, c, :P]    = sum_{n < n_k} r_eta,n a_n - lam_k beta
 *   gcut_j         = sum_{n < n_k} ([y_n = j + 1] u_lo,n + [y_n = j] u_hi,n)
 *   G[k, c, P]     = sum_{j >= 0} gcut_j - kap_k delta_0
 *   G[k, c, P + i] = e^{delta_i} sum_{j >= i} gcut_j - kap_k delta_i          (i = 1 .. C - 2)
 * No two probabilities are subtracted: the gap w is e^{delta_y} itself and log(1 - e^{-w}) is a proper log1mexp.  For C = 2 the
 * model is logistic regression on the design [A, -1] with the intercept's prior precision kap.  A (K x N x P) doubles, y (K x N)
 * ints, offset (K x N), X, G (K x nc x D), lp (K x nc), packed, in device memory; C >= 2, P >= 1, D <= 64; K, nc, N, counts_dev and
 * prior_prec / prior_prec_dev (lam, the prior N(0, I / lam_k) of beta) as in gsmvi_glm_batched_f64; cut_prec / cut_prec_dev (kap,
 * finite and >= 0; 0 = flat) in the same scalar-or-K-values style: the prior N(0, I / kap_k) of delta.  At least one of G, lp is
 * given.  Every output row sums over n in the order 0 .. n_k - 1 in one thread, the suffix sums over j run from C - 2 downwards, and
 * a row depends on its problem and its own row of X only: the same bits for any K, nc and neighbours; no atomics.  Rows n >= n_k are
 * never loaded; n_k = 0 leaves the two priors.  A label outside 0 .. C - 1 cannot be checked on this side of the ABI: the kernel
 * clamps it, so it reads nothing out of bounds (the range is the caller's to keep).  A row of X with a non-finite entry, or in which
 * some e^{delta_j}, j >= 1, is not a positive normal number (|delta_j| above 708), gets NaN outputs and no other row is touched;
 * delta_0 is a location and is not limited.  Shapes, priors, NULL arrays and overlaps (G and lp are the written arrays) are checked
 * before the context is looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs
 * are only read; no context workspace; one capturable launch.  Sets GSMVI_PATH_BATCHED_TARGET.
 */
int gsmvi_ordinal_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int nc, int64_t N, const double* A,
                              const int* y, const double* offset, const int* counts_dev, double prior_prec,
                              const double* prior_prec_dev, double cut_prec, const double* cut_prec_dev, const double* X, double* G,
                              double* lp);

/*
 * Batched softmax target: the log-density and the score of K Bayesian multinomial logit regressions of one (N, C, P) at nc points
 * each, one launch.  examples/example_gsm.py:34-35, the model's log_prob and lp_g = jit(grad(...)) of it, for a response with C
 * classes -> gsmvi_softmax_batched_f64.  Problem k has the design matrix A_k (N rows a_n of P features), integer labels y_kn in
 * 0 .. C - 1, n_k valid rows and prior precision lam_k >= 0 (prior N(0, I / lam_k); 0 = flat).  Class C - 1 is the reference class
 * with zero coefficients; the parameter is x in R^D, D = (C - 1) P, laid out class-major: x[c P + j] = W_cj.  At a row x of X_k:
 *   eta_nc = a_n . w_c  (c < C-1),   eta_n,C-1 = 0
 *   m_n    = max_c eta_nc            (over all C values, the 0 included)
 *   s_n    = sum_{c=0..C-1} exp(eta_nc - m_n)     (class order; the reference class last)
 *   lp(x)  = sum_{n<n_k} [ eta_n,y_n - m_n - log s_n ] - lam_k |x|^2 / 2
 *   g_cj   = sum_{n<n_k} ( [y_n = c] - exp(eta_nc - m_n)/s_n ) a_nj - lam_k x_cj      (c < C-1)
 * The term of the first class that attains m_n is exactly 1, so every softmax entry point sums the other terms alone (rest_n),
 * takes s_n = 1 + rest_n and evaluates log s_n as log1p(rest_n): where the reference class (or any other) wins by more than
 * 1 / eps, s_n rounds to 1 and log(s_n) would return 0 for a term that is -rest_n.
 * A (K x N x P) doubles, labels (K x N) ints, X, G (K x nc x D), lp (K x nc), packed, in device memory.  C >= 2, P >= 1,
 * 1 <= D <= 64 and K with the grid limits of the batched GSM above; nc >= 1 and N >= 1 are not bounded by LDS (both are walked in
 * tiles; the tile of X rows shrinks as C grows).  counts_dev: NULL = N valid rows everywhere, else K ints on the device, each
 * clamped to 0 .. N in the kernel; rows n >= n_k are never loaded, whatever they hold.  prior_prec_dev: NULL = the scalar prior_prec
 * (finite, >= 0) for every problem, else K values.  At least one of G, lp is given; G alone evaluates no logarithm, lp alone makes
 * no second pass over a tile.  Every output row sums over n in the order 0 .. n_k - 1 in one thread and depends on A_k, y_k, n_k,
 * lam_k and its own row of X only: the same bits for any K, nc, tiling and neighbours.  A row of X with a non-finite entry, or for
 * which some valid eta is not finite, gets NaN outputs and no other row is touched.  The maximum is subtracted, so nothing else can
 * overflow.  A label is used in comparisons and selects only, never as an index: a label outside 0 .. C - 1 reads nothing out of
 * bounds (its row counts as one whose class has eta = 0 and no residual indicator; the ranges are the caller's to keep).  Shapes,
 * NULL arrays, the scalar prior and overlaps (G and lp are the written arrays) are checked before the context is looked at (then a
 * NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is
 * used; one capturable launch.  Sets GSMVI_PATH_BATCHED_SOFTMAX.
 */
int gsmvi_softmax_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int nc, int64_t N, const double* A,
                              const int* labels, const int* counts_dev, double prior_prec, const double* prior_prec_dev,
                              const double* X, double* G, double* lp);

/*
 * Batched L-BFGS initialiser (gsmvi/initializers.py:5-17 for K problems of one D): the minimiser of phi_k = -lp_k as the mean and
 * the dense BFGS inverse-Hessian product of the stored pairs on an identity base (scipy.optimize.LbfgsInvHessProduct(S, Y)
 * .todense(), what res.hess_inv.todense() is) as the covariance.  Plain L-BFGS, history 10, Armijo backtracking (c1 = 1e-4,
 * halving, at most 20 rejected trials per search); not a port of L-BFGS-B (no bounds, no Cauchy point, no More-Thuente search).
 * 1 <= D <= 64, K >= 1 with the grid limits of the batched GSM above.  State, caller-owned, packed, in device memory:
 *   x, g, d (K x D)  the last accepted point, the gradient of phi there, the search direction
 *   S, Y (K x 10 x D) ring buffers of the pairs s = x' - x, y = g' - g; the held pairs are the slots head - n .. head - 1 (mod 10)
 *   sc (K x 24)      [0] f = phi(x), [1] the trial step t, [2] g.d, [3] spare, [4..13] s.y of the ten slots, [14..23] y.y
 *   ist (K x 8)      [0] status (0 running, 1 converged, 2 maxiter / maxfun reached, 3 line search failed, 4 non-finite start),
 *                    [1] nit, [2] nfev, [3] nls (rejected trials of this search), [4] n = pairs held, [5] head = next slot, [6..7] spare
 *   Xt (K x D)       the trial point: where the caller evaluates lp and its score next (K x 1 x D for the batched callables)
 * gsmvi_lbfgs_step_batched_f64, one launch per evaluation.  ft = sign fv[k], gt = sign gv[k] (sign = -1: fv, gv are lp and its
 * score at Xt; sign = 1: phi and its gradient).  start != 0: x holds x0 and Xt a copy of it; every other entry of the state is
 * written: nfev = 1; non-finite ft or gt -> status 4; max|g| <= gtol -> status 1; else d = -g, t = min(1, 1 / |g|_2), g.d, Xt = x + t d.
 * start == 0, for every problem with status 0: nfev += 1; ok = ft, gt finite and ft <= f + (1e-4 t) (g.d).  Not ok: t <- t / 2,
 * nls += 1; nls > 20 -> status 3; else nfev >= maxfun -> status 2; else Xt = x + t d.  Ok: s = Xt - x, y = gt - g, (x, f, g) <- (Xt,
 * ft, gt), nit += 1, the pair goes to slot head iff s.y > 2.2e-16 y.y; then max|g| <= gtol or fprev - f <= ftol max(|fprev|, |f|, 1)
 * -> status 1; else nit >= maxiter or nfev >= maxfun -> status 2; else d = -H g by the two-loop recursion (scale s.y / y.y of the
 * newest pair), t = 1 (no pair held, or g.d not < 0, which also drops the history: the steepest-descent start above), nls = 0,
 * Xt = x + t d.  A problem whose status is not 0 is frozen: nothing of it is written.  *stopped_dev (one int, may be NULL) grows by
 * the number of problems that stopped in this launch.  Every dot product is summed in an order fixed by D alone, so a problem's
 * bits do not depend on K or on its neighbours.  maxiter >= 1, maxfun >= 2, gtol, ftol >= 0.  Written: the state and
 * *stopped_dev, none of which may overlap any other array of the call.
 * gsmvi_lbfgs_hess_inv_batched_f64: cov_k (K x D x D) = H after H_0 = I and, over the held pairs from oldest to newest with
 * rho = 1 / s.y, H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T; exactly symmetric; the identity when no pair is held.  Reads
 * S, Y and ist[4], ist[5] only.
 * Both: shapes, NULL arrays and overlaps are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  No context workspace is used.  Sets GSMVI_PATH_BATCHED_LBFGS.
 */
int gsmvi_lbfgs_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int start, const double* fv, const double* gv,
                                 double sign, double* x, double* g, double* d, double* S, double* Y, double* sc, int* ist,
                                 double* Xt, int* stopped_dev, int maxiter, int maxfun, double gtol, double ftol);
int gsmvi_lbfgs_hess_inv_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, const double* S, const double* Y,
                                     const int* ist, double* cov);

/*
 * Batched Pathfinder initialiser, single-path form (Zhang, Carpenter, Gelman, Vehtari 2022): the role of gsmvi/initializers.py:5-17
 * (a mean and a covariance to start a fit from) with a start that is picked by how well it fits.  Every accepted iterate of the
 * batched L-BFGS above defines a Gaussian from the pairs held at that moment; M draws estimate its ELBO; the best is kept.  Two
 * launches per L-BFGS round, one before and one after the caller's lp of the draws.  1 <= D <= 64, 1 <= M <= 4096, K >= 1 with the
 * grid limits of the batched GSM above.  All arrays packed, in device memory.
 * gsmvi_pathfinder_propose_batched_f64 reads the L-BFGS state (x, g, S, Y, sc, ist as laid out above), seeds (K stream keys) and
 * seen (K ints; the caller starts them at -1, so the start point is path point 0).  Per problem: fresh[k] = (ist[1] = nit != seen[k]),
 * then seen[k] <- nit.  Not fresh (a rejected trial, a frozen problem): the M rows of X_k <- x_k (so that the lp that follows reads
 * defined memory), logq_sum[k] <- NaN, and nothing else of problem k is written.  Fresh: gamma = h0 if h0 > 0, else s.y / y.y of
 * the newest held pair (sc[4 + i] / sc[14 + i], i = head - 1 mod 10; 1 with no pair held); Sigma = H after H_0 = gamma I and, over
 * the held pairs from oldest to newest with rho = 1 / s.y, H <- (I - rho s y^T) H (I - rho y s^T) + rho s s^T -- the recursion of
 * gsmvi_lbfgs_hess_inv_batched_f64 in the same operations (h0 = 1 gives its bits), exactly symmetric; mu = x - Sigma g (g is the
 * gradient of phi = -lp, as the state holds it); R = chol(Sigma), upper; z = the rows 0 .. M - 1 of draw `call` = nit of the problem's
 * stream in the plain layout of gsmvi_kl_draw_batched_f64 (element s D + j, pair (s D + j) / 2, no odd-D padding); X_k row s = mu +
 * z_s R; logq_sum[k] = sum_s (-|z_s|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi); mu (K x D), cov (K x D x D) = Sigma and info[k] = 0,
 * or 1 + the first pivot that is not > 0 and finite, are written.  A bad pivot or a mean that is not finite (a non-finite gradient)
 * gives NaN rows and a NaN logq_sum[k]; no other problem is touched.  The base gamma I in place of the paper's diagonal alpha is a
 * stated simplification.
 * gsmvi_pathfinder_select_batched_f64: e = (lpsum[k] - logq_sum[k]) / M for fresh[k] != 0 and info[k] = 0, NaN otherwise;
 * elbo_last[k] = e; npts[k] += (fresh[k] != 0); e finite and e > best_elbo[k] (strict: the first maximum wins) -> best_elbo[k] = e,
 * best_mean_k = mu_k, best_cov_k = cov_k, best_it[k] = ist[1]; otherwise nothing of the problem's best state is written.
 * Both: every sum runs in an order fixed by (D, M) alone, so a problem's bits depend neither on K nor on its neighbours.  Shapes,
 * NULL arrays and overlaps (a written array may overlap no other array of the call) are checked before the context is looked at
 * (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  No context workspace is used; one
 * capturable launch each.  Sets GSMVI_PATH_BATCHED_PATHFINDER.
 */
int gsmvi_pathfinder_propose_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, const double* x,
                                         const double* g, const double* S, const double* Y, const double* sc, const int* ist,
                                         const uint64_t* seeds, int* seen, double h0, int* fresh, double* mu, double* cov,
                                         double* X, double* logq_sum, int* info);
int gsmvi_pathfinder_select_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, const double* lpsum,
                                        const double* logq_sum, const int* fresh, const int* info, const int* ist, const double* mu,
                                        const double* cov, double* elbo_last, int* npts, double* best_elbo, double* best_mean,
                                        double* best_cov, int* best_it);

/*
 * Batched Laplace initialiser: the Newton mode of K GLM posteriors of one (N, D) and the inverse of the negative Hessian there
 * as the covariance.  The reference has no Laplace initialiser: this fills the role of gsmvi/initializers.py:5-17 (the maximiser
 * of lp as the mean, an inverse-Hessian estimate as the covariance) for the models of examples/example_gsm.py:34-35 whose second
 * derivative is closed-form, the four families of gsmvi_glm_batched_f64.  With eta_n = a_n . x + o_kn and the weight
 *   w = -dr / d eta:   logistic  sigma (1 - sigma) = e / (1 + e)^2, e = exp(-|eta|)      poisson  e^eta      gaussian  tau_k
 *                      probit    y hp (hp + eta) + (1 - y) hm (hm - eta), hp = phi / Phi(eta), hm = phi / Phi(-eta)
 * (probit: the tail side, hp + eta at eta < 0 and hm - eta at eta > 0, cancels: formed by subtraction its relative error grows
 * like eps eta^2 until it is the whole value, so from |eta| = 4 on it is g (1 + g / eta^2), g = 1 / (1 + 2 / eta^2 / (1 + 3 / eta^2 / ..))
 * from the continued fraction of the Mills ratio, without a subtraction; 0 <= w <= 1 for every finite eta),
 *   H_k(x) = sum_{n < n_k} w(eta_n, y_n) a_n a_n^T + lam_k I         the negative Hessian of lp_k at x, positive semi-definite.
 * The argument meanings, bounds and grid limits of gsmvi_glm_batched_f64 hold for both entry points (1 <= D <= 64, any N >= 1,
 * counts_dev clamped in the kernel and rows n >= n_k never loaded, noise_prec the gaussian family's alone).  The Gram product runs
 * on the fp64 MFMA over tiles of 32 rows; every sum over n is taken in an order fixed by (N, D) alone, so a problem's bits depend
 * on its own data only, not on K or its neighbours.
 *
 * gsmvi_glm_hessian_batched_f64: at the rows x_k of X (K x D), H (K x D x D, or NULL) = H_k(x_k), exactly symmetric (one triangle
 * is computed and mirrored); cov (K x D x D, or NULL) = H_k^{-1} through a Cholesky factorisation, exactly symmetric; info_dev
 * (K ints, required with cov and only with it): 0, or 1 + the index j of the first pivot that is not finite or not > 64 eps H_jj
 * (a relative rule: a rank-deficient H fails whatever the rounding), and then cov_k is the identity (nothing is known: what
 * gsmvi_lbfgs_hess_inv_batched_f64 gives without a pair).  A non-finite x_k or (poisson) a valid row whose e^eta is not finite
 * gives H_k = NaN, info[k] = 1, cov_k = I, and no other problem is touched.  At least one of H, cov is given.
 *
 * gsmvi_laplace_step_batched_f64: one launch is one damped Newton round of phi_k = -lp_k for every running problem.  State,
 * caller-owned, packed, in device memory, laid out like the L-BFGS state above:
 *   x, g, d, Xt (K x D)  the last accepted point, the gradient of phi there, the Newton direction, the trial point
 *   sc (K x 4)           [0] f = phi(x), [1] the trial step t, [2] g.d, [3] spare
 *   ist (K x 8)          [0] status (0 running, 1 converged, 2 maxiter / maxfun reached, 3 line search failed, 4 non-finite start,
 *                        5 H not positive definite), [1] nit, [2] nfev, [3] nls (rejected trials of this search), [4..7] spare
 * Per running problem the launch evaluates ft, gt and H at Xt in one sweep over A_k.  start != 0 (Xt holds x0; every entry of the
 * state is written): x = Xt, nfev = 1; ft or gt not finite -> status 4; max|g| <= gtol -> status 1; else H is factored (failure by
 * the pivot rule above -> status 5) and d = -H^{-1} g, t = 1, g.d, Xt = x + d.  start == 0: nfev += 1; ok = ft, gt finite and
 * ft <= f + (1e-4 t) (g.d) + 1e-10 max(1, |f|) (the slack keeps the test decidable where the decrease of f is below its own
 * rounding).  Not ok: t <- t / 2, nls += 1; nls > 20 -> status 3; else nfev >= maxfun -> status 2; else Xt = x + t d.  Ok: (x, f, g)
 * <- (Xt, ft, gt), nit += 1; max|g| <= gtol -> status 1; else nit >= maxiter or nfev >= maxfun -> status 2; else H(x) is factored
 * (failure -> status 5) and d = -H^{-1} g, t = 1, nls = 0, g.d, Xt = x + d.  A problem whose status is not 0 is frozen: nothing of
 * it is written and nothing of A_k is loaded for it.  *stopped_dev (one int, may be NULL) grows by the number of problems that
 * stopped in this launch.  maxiter >= 1, maxfun >= 2, gtol >= 0.  Written: the state and *stopped_dev, none of which may overlap
 * any other array of the call.
 * Both: shapes, NULL arrays and overlaps are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is used.  Sets
 * GSMVI_PATH_BATCHED_LAPLACE.
 */
int gsmvi_glm_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                  const double* y, const double* offset, const int* counts_dev, double noise_prec,
                                  const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, const double* X,
                                  double* H, double* cov, int* info_dev);
int gsmvi_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                   const double* y, const double* offset, const int* counts_dev, double noise_prec,
                                   const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, int start,
                                   double* x, double* g, double* d, double* sc, int* ist, double* Xt, int* stopped_dev, int maxiter,
                                   int maxfun, double gtol);

/*
 * Batched softmax Laplace initialiser: the Newton mode of K multinomial logit posteriors of one (N, C, P) and the inverse of the
 * negative Hessian there as the covariance.  The reference has no Laplace initialiser: this fills the role of
 * gsmvi/initializers.py:5-17 (the maximiser of lp as the mean, an inverse-Hessian estimate as the covariance) for the multinomial
 * logit model of gsmvi_softmax_batched_f64, given to the reference as log_prob and jit(grad(...)) of it
 * (examples/example_gsm.py:34-35).  With that entry's parametrisation (class C - 1 the reference class, eta = 0; x[c P + j] = W_cj;
 * D = (C - 1) P <= 64), its m_n and s_n, and p_nc = exp(eta_nc - m_n) / s_n, for d = c P + i and d' = c' P + j, c, c' < C - 1:
 *   H_k(x)[d, d'] = sum_{n < n_k} w_n,cc' a_ni a_nj + lam_k [d = d']      the negative Hessian of lp_k at x, positive semi-definite
 *   w_n,cc  = p_nc (1 - p_nc),   w_n,cc' = -p_nc p_nc'  (c != c'),   phi = -lp,   g = -score,   d_newton = -H^{-1} g.
 * 1 - p_nc is a sum over the other classes: with c* the first class that attains m_n (e_c* = 1 exactly), s_rest = sum_{c != c*} e_c
 * and s = 1 + s_rest, 1 - p_c* = s_rest / s and 1 - p_c = (s - e_c) / s for c != c* (s - e_c >= 1); the reference class takes part
 * in m, s and s_rest like any other.  It is never 1.0 - p and never a difference of two Gram sums, which lose every digit of a
 * diagonal class block when one class saturates.  The residual of the gradient is 1 - p_nc in that form where y_n = c and -p_nc
 * elsewhere.  The argument meanings, bounds and grid limits of gsmvi_softmax_batched_f64 hold for both entry points (C >= 2, P >= 1,
 * any N >= 1, counts_dev clamped in the kernel and rows n >= n_k never loaded, a label used in comparisons only).  The Gram
 * product runs on the fp64 MFMA over tiles of 32 rows; every sum over n is taken in an order fixed by (N, C, P) alone, so a
 * problem's bits depend on its own data only, not on K or its neighbours.
 *
 * gsmvi_softmax_hessian_batched_f64: H, cov and info_dev as gsmvi_glm_hessian_batched_f64 gives them, at the rows x_k of X (K x D).
 * A non-finite x_k or a valid row with a non-finite eta gives H_k = NaN, info[k] = 1, cov_k = I (by a flag, not by arithmetic), and
 * no other problem is touched.  At least one of H, cov is given; info_dev is required with cov and only with it.
 *
 * gsmvi_softmax_laplace_step_batched_f64: one launch is one damped Newton round of phi_k = -lp_k for every running problem: the
 * state (x, g, d, Xt (K x D), sc (K x 4), ist (K x 8)), the status codes, the Armijo test with its slack, the halving, the 20
 * rejections, *stopped_dev and the meaning of start, maxiter, maxfun and gtol are those documented for
 * gsmvi_laplace_step_batched_f64, word for word; a non-finite x or eta is status 4 at the start and a rejected trial later.
 * Both: shapes, NULL arrays and overlaps are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is used; at most 64 KB of dynamic
 * LDS (no kernel attribute).  Sets GSMVI_PATH_BATCHED_SOFTMAX_LAPLACE.
 */
int gsmvi_softmax_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, const double* A,
                                      const int* labels, const int* counts_dev, double prior_prec, const double* prior_prec_dev,
                                      const double* X, double* H, double* cov, int* info_dev);
int gsmvi_softmax_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, const double* A,
                                           const int* labels, const int* counts_dev, double prior_prec,
                                           const double* prior_prec_dev, int start, double* x, double* g, double* d, double* sc,
                                           int* ist, double* Xt, int* stopped_dev, int maxiter, int maxfun, double gtol);

/*
 * Shared-design Laplace initialiser: the Newton mode of K GLM posteriors over ONE design matrix and the inverse of the negative
 * Hessian there as the covariance: the two entry points above for the model of gsmvi_glm_shared_batched_f64 (the role of
 * gsmvi/initializers.py:5-17 for the models of examples/example_gsm.py:34-35; no reference twin).  A is (N x D), shared; y, offset
 * (NULL = none) and weights (NULL = 1 everywhere) are (K x N); weights v_kn >= 0 are observation weights.  With eta_n = a_n . x +
 * o_kn, the link (r, t) of gsmvi_glm_batched_f64 and the weight w = -dr / d eta of gsmvi_glm_hessian_batched_f64:
 *   f_k(x) = -( sum_n v_kn t(eta_n, y_kn) - lam_k |x|^2 / 2 )       g_k(x) = -( sum_n v_kn r(eta_n, y_kn) a_n - lam_k x )
 *   H_k(x) =    sum_n v_kn w(eta_n, y_kn) a_n a_n^T + lam_k I       positive semi-definite, since v >= 0.
 * An observation whose weight is not > 0 is removed by selection, not by a product with zero: it contributes exactly nothing to f,
 * g and H whatever y, offset and eta hold there (a NaN y, an infinite offset, an e^eta that overflows) and flags nothing.  A is
 * never replicated: one tile of 32 rows of A is staged in LDS per workgroup and serves every problem of that workgroup (four for
 * D <= 16, one above), and nothing of size K N D exists anywhere.  Every sum over n runs n = 0 .. N - 1 in tiles of 32, the Gram
 * product on the fp64 MFMA, in an order fixed by (N, D) alone: a problem's bits depend on its own data only, not on K, its
 * position or its neighbours.  The bounds of gsmvi_glm_shared_batched_f64 at nc = 1 hold (1 <= D <= 64, any N >= 1, K within the
 * packing of gsmvi_glm_hessian_batched_f64), noise_prec is the gaussian family's alone.
 *
 * gsmvi_glm_shared_hessian_batched_f64: H (K x D x D, or NULL), cov (K x D x D, or NULL) and info_dev (K ints, required with cov and
 * only with it) as gsmvi_glm_hessian_batched_f64 gives them, at the rows x_k of X (K x D): H exactly symmetric, the pivot rule
 * 64 eps H_jj, cov_k = I where the factorisation fails.  A non-finite x_k, or (poisson) an e^eta that is not finite at an
 * observation with v > 0, gives H_k = NaN, info[k] = 1, cov_k = I, and no other problem is touched; a non-finite entry of A
 * reaches every problem.  At least one of H, cov is given.
 *
 * gsmvi_laplace_shared_step_batched_f64: one launch is one damped Newton round of phi_k = f_k for every running problem: the state
 * (x, g, d, Xt (K x D), sc (K x 4), ist (K x 8)), the status codes 1 - 5, the Armijo test with its slack 1e-10 max(1, |f|), the
 * halving, the 20 rejections, *stopped_dev and the meaning of start, maxiter, maxfun and gtol are those documented for
 * gsmvi_laplace_step_batched_f64, word for word; a flagged trial point is status 4 at the start and a rejected trial later.  A
 * problem whose status is not 0 is frozen: nothing of it is written and nothing of y, offset or weights is loaded for it; a
 * workgroup all of whose problems are frozen leaves after reading the status words.
 * Both: shapes, NULL arrays and overlaps (only the written arrays may not overlap anything) are checked before the context is
 * looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no
 * context workspace is used; at most 64 KB of dynamic LDS (no kernel attribute).  Both set GSMVI_PATH_BATCHED_LAPLACE |
 * GSMVI_PATH_BATCHED_TARGET: only the two negative binomial entry points below set that pair too (all 32 bits are taken), so
 * gsmvi_last_path still proves that a batched Laplace kernel with a model of its own ran.
 */
int gsmvi_glm_shared_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                         const double* y, const double* offset, const double* weights, double noise_prec,
                                         const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev,
                                         const double* X, double* H, double* cov, int* info_dev);
int gsmvi_laplace_shared_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t N, int family, const double* A,
                                          const double* y, const double* offset, const double* weights, double noise_prec,
                                          const double* noise_prec_dev, double prior_prec, const double* prior_prec_dev, int start,
                                          double* x, double* g, double* d, double* sc, int* ist, double* Xt, int* stopped_dev,
                                          int maxiter, int maxfun, double gtol);

/*
 * Negative binomial Laplace initialiser: the Newton mode of K negative binomial posteriors and the inverse of the negative Hessian
 * there as the covariance: the two entry points above for the model of gsmvi_negbin_batched_f64, whose arguments (K, P, N, A, y,
 * offset, counts_dev, theta_mean, theta_prec, prior_prec and their _dev forms) and bounds at nc = 1 they take (the role of
 * gsmvi/initializers.py:5-17 for the model of examples/example_gsm.py:34-35; no reference twin).  x = (beta, theta), D = P + 1 <= 64,
 * r = e^theta, d = eta - theta, sigma = sigma(d); with (t, r_eta, r_theta) of gsmvi_negbin_batched_f64, dps = psi(y + r) - psi(r)
 * and dtg = psi'(y + r) - psi'(r), each formed as one difference and never from two calls:
 *   w_ee = (y + r) sigma(d) sigma(-d) >= 0      w_et = -sigma r_eta      w_tt = -[ r (dps - softplus(d)) + r^2 dtg + r sigma - sigma r_eta ]
 *   f_k(x) = -lp_k(x),   g_k(x) = -score_k(x),
 *   H_k[:P, :P] = sum_{n < n_k} w_ee,n a_n a_n^T + lam_k I     H_k[:P, P] = sum_{n < n_k} w_et,n a_n     H_k[P, P] = sum_{n < n_k} w_tt,n + kap_k
 * H_k is the negative Hessian of lp_k.  It is NOT positive semi-definite in general: w_tt has any sign, and lp_k is not concave
 * in theta.  The P x P block and the border column are one Gram product on the fp64 MFMA over tiles of 32 rows; H[P, P] is summed
 * in order by one thread.  Every sum over n runs in an order fixed by (N, P) alone: a problem's bits depend on its own data only.
 *
 * gsmvi_negbin_hessian_batched_f64: H (K x D x D, or NULL), cov (K x D x D, or NULL) and info_dev (K ints, required with cov and only
 * with it) as gsmvi_glm_hessian_batched_f64 gives them, at the rows x_k of X (K x D): H exactly symmetric, the pivot rule
 * 64 eps H_jj, cov_k = I and info[k] = 1 + the first failing pivot where H_k is not positive definite (nothing is modified here).  A
 * non-finite x_k, or an e^theta that is not a positive normal number, gives H_k = NaN, info[k] = 1, cov_k = I, and no other problem
 * is touched.  At least one of H, cov is given.
 *
 * gsmvi_negbin_laplace_step_batched_f64: one launch is one damped Newton round of phi_k = f_k for every running problem: the state
 * (x, g, d, Xt (K x D), sc (K x 4), ist (K x 8)), the status codes 1 - 5, the Armijo test with its slack 1e-10 max(1, |f|), the
 * halving, the 20 rejections, *stopped_dev and the meaning of start, maxiter, maxfun and gtol are those documented for
 * gsmvi_laplace_step_batched_f64; a flagged trial point is status 4 at the start and a rejected trial later.  One rule is this entry
 * point's own, the last-pivot rule: when the factorisation for a new direction fails at exactly the last pivot (info = D: no
 * positive curvature in theta given beta), with R the factor, s = H[P, P] - sum_{c < P} R[c, P]^2 and m = |H[P, P]| + sum_{c < P}
 * R[c, P]^2 (both in c order), and |s| finite and > 64 eps m, the last pivot is replaced by sqrt|s|, the round goes on as if the
 * factorisation had succeeded (the modified matrix is positive definite, so d is a descent direction) and ist[4], zero at the
 * start, grows by one: the rounds with a modified pivot.  A pivot that fails before the last, or an |s| below that bar, is
 * status 5 as before.  A problem whose status is not 0 is frozen: nothing of it is written and nothing of A_k is loaded for it.
 * Both: shapes, NULL arrays and overlaps (only the written arrays may not overlap anything) are checked before the context is
 * looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no
 * context workspace is used; at most 64 KB of dynamic LDS (no kernel attribute).  Both set GSMVI_PATH_BATCHED_LAPLACE |
 * GSMVI_PATH_BATCHED_TARGET, the pair of the shared-design entry points above.
 */
int gsmvi_negbin_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t N, const double* A, const double* y,
                                     const double* offset, const int* counts_dev, double theta_mean, const double* theta_mean_dev,
                                     double theta_prec, const double* theta_prec_dev, double prior_prec,
                                     const double* prior_prec_dev, const double* X, double* H, double* cov, int* info_dev);
int gsmvi_negbin_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t N, const double* A,
                                          const double* y, const double* offset, const int* counts_dev, double theta_mean,
                                          const double* theta_mean_dev, double theta_prec, const double* theta_prec_dev,
                                          double prior_prec, const double* prior_prec_dev, int start, double* x, double* g,
                                          double* d, double* sc, int* ist, double* Xt, int* stopped_dev, int maxiter, int maxfun,
                                          double gtol);

/*
 * Ordinal Laplace initialiser: the Newton mode of K cumulative-logit posteriors and the inverse of the negative Hessian there as the
 * covariance: the two entry points above for the model of gsmvi_ordinal_batched_f64, whose arguments (K, P, C, N, A, y (int labels),
 * offset, counts_dev, prior_prec, cut_prec and their _dev forms) and bounds at nc = 1 they take (the role of
 * gsmvi/initializers.py:5-17 for the model of examples/example_gsm.py:34-35; no reference twin).  x = (beta, delta),
 * D = P + C - 1 <= 64, w_0 = 1, w_i = e^{delta_i} (i >= 1), q_i = 1 / expm1(w_i); with a, b, t, r_eta of gsmvi_ordinal_batched_f64,
 * fa = sigma(a) sigma(-a) (0 for y = 0), fb = sigma(b) sigma(-b) (0 for y = C - 1) and, per (row n, cutpoint i),
 *   e_ni = fa + fb (i < y_n), fb (i = y_n), 0 (i > y_n)        s_ni = -r_eta,n (i < y_n), sigma(-b_n) (i = y_n), 0 (i > y_n)
 *   F(i) = sum_{n < n_k} e_ni     S_i = sum_{n < n_k} s_ni + q_i cnt_i     cnt_i = #{n < n_k : y_n = i}  (1 <= i <= C - 2, else 0)
 *   f_k(x) = -lp_k(x),   g_k(x) = -score_k(x) = -( sum_n r_eta,n a_n - lam_k beta,  w_i S_i - kap_k delta_i ),
 *   H_k[:P, :P] = sum_{n < n_k} (fa + fb)_n a_n a_n^T + lam_k I          H_k[:P, P + i] = -w_i sum_{n < n_k} e_ni a_n
 *   H_k[P + i, P + i'] = w_i w_i' F(max(i, i'))  (i != i')
 *   H_k[P + i, P + i]  = w_i^2 F(i) + (w_i q_i) (w_i + w_i q_i) cnt_i + c_i + kap_k,     c_i = -w_i S_i (i >= 1), c_0 = 0
 * H_k is the negative Hessian of lp_k, built in the gap coordinates (delta_0, w_1 .. w_{C-2}) as a sum of positive semi-definite
 * terms: no two probabilities are subtracted.  The chain terms c_i make it indefinite away from the mode.  The P x P block and the
 * border block are one Gram product on the fp64 MFMA over tiles of 32 rows; F, S and cnt are summed in order by one thread each.
 * Every sum over n runs in an order fixed by (N, P, C) alone: a problem's bits depend on its own data only.  Labels are clamped to
 * 0 .. C - 1 as staged; rows n >= n_k are never loaded.
 *
 * gsmvi_ordinal_hessian_batched_f64: H (K x D x D, or NULL), cov (K x D x D, or NULL) and info_dev (K ints, required with cov and
 * only with it) as gsmvi_glm_hessian_batched_f64 gives them, at the rows x_k of X (K x D): H exactly symmetric, the pivot rule
 * 64 eps H_jj, cov_k = I and info[k] = 1 + the first failing pivot where H_k is not positive definite (nothing is modified here).  A
 * non-finite x_k, or some e^{delta_j}, j >= 1, that is not a positive normal number, gives H_k = NaN, info[k] = 1, cov_k = I, and no
 * other problem is touched.  At least one of H, cov is given.
 *
 * gsmvi_ordinal_laplace_step_batched_f64: one launch is one damped Newton round of phi_k = f_k for every running problem: the state
 * (x, g, d, Xt (K x D), sc (K x 4), ist (K x 8)), the status codes 1 - 5, the Armijo test with its slack 1e-10 max(1, |f|), the
 * halving, the 20 rejections, *stopped_dev and the meaning of start, maxiter, maxfun and gtol are those documented for
 * gsmvi_laplace_step_batched_f64; a flagged trial point is status 4 at the start and a rejected trial later.  One rule is this entry
 * point's own, the retry rule: when the factorisation for a new direction fails (any pivot) and some c_i < 0, every diagonal entry
 * H[P + i, P + i] is replaced by H[P + i, P + i] - min(c_i, 0) (the pivot rule's reference diagonal follows) and the matrix is
 * factored once more; on success the round goes on as if the factorisation had succeeded (the retried matrix is positive
 * semi-definite plus the priors, so d is a descent direction) and ist[4], zero at the start, grows by one: the rounds whose
 * direction came from the retried matrix.  No negative c_i, or a second failure, is status 5 as before.  A problem whose status is
 * not 0 is frozen: nothing of it is written and nothing of A_k is loaded for it.
 * Both: shapes, priors, NULL arrays and overlaps (only the written arrays may not overlap anything) are checked before the context
 * is looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no
 * context workspace is used; at most 64 KB of dynamic LDS (no kernel attribute).  Both set GSMVI_PATH_BATCHED_LAPLACE |
 * GSMVI_PATH_BATCHED_TARGET, the pair of the shared-design and negative binomial entry points above.
 */
int gsmvi_ordinal_hessian_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t N, const double* A,
                                      const int* y, const double* offset, const int* counts_dev, double prior_prec,
                                      const double* prior_prec_dev, double cut_prec, const double* cut_prec_dev, const double* X,
                                      double* H, double* cov, int* info_dev);
int gsmvi_ordinal_laplace_step_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t N, const double* A,
                                           const int* y, const double* offset, const int* counts_dev, double prior_prec,
                                           const double* prior_prec_dev, double cut_prec, const double* cut_prec_dev, int start,
                                           double* x, double* g, double* d, double* sc, int* ist, double* Xt, int* stopped_dev,
                                           int maxiter, int maxfun, double gtol);

/*
 * Batched GLM posterior predictive: what a fitted q_k = N(mean_k, cov_k) over the coefficients of K GLMs of one D says about M new
 * rows per problem, one launch.  examples/example_gsm.py:34-35 builds the model and the reference stops at the fitted (mean, cov):
 * this is the use of the fit (predictions and the held-out score, the expected log predictive density), with no reference twin.
 * The model's arguments are those of gsmvi_glm_hessian_batched_f64 with the number of new rows M in place of N and no prior:
 * family, A (K x M x D), offset (K x M or NULL), y (K x M or NULL), counts_dev (K ints or NULL, clamped to 0 .. M in the kernel),
 * noise_prec / noise_prec_dev (the gaussian family's alone: 1.0 and NULL for any other).  mean (K x D) and cov (K x D x D, read as
 * given, both triangles) are the posterior.  Q (1 <= Q <= 64) and gh_t, gh_logw (Q doubles each, on the device) are the
 * Gauss-Hermite nodes and the logarithms of their weights (numpy.polynomial.hermite.hermgauss; no table lives in the library).
 * For row n < n_k of problem k:
 *   m = a_n . mean_k + o_kn,   v = a_n^T cov_k a_n,   v+ = max(v, 0),   s = sqrt(2 v+),   eta_q = m + s t_q
 *   eta_mean = m,  eta_var = v (the raw value: a covariance that is not positive semi-definite shows), and
 *   family     pmean = E[E[y | eta]]                        lpd = log E[p(y | eta)]  (normalised)
 *   gaussian   m                                            -log(2 pi (v+ + 1 / tau_k)) / 2 - (y - m)^2 / (2 (v+ + 1 / tau_k))
 *   probit     Phi(m / sqrt(1 + v+))  (through erfc)        LSE_q(logw_q + t(eta_q, y)) - log(pi) / 2
 *   poisson    exp(m + v+ / 2)                              LSE_q(logw_q + y eta_q - e^eta_q) - log(pi) / 2 - lgamma(y + 1)
 *   logistic   sum_q exp(logw_q) sigma(eta_q) / sqrt(pi)    LSE_q(logw_q + t(eta_q, y)) - log(pi) / 2
 * with t the family's t of gsmvi_glm_batched_f64 above, LSE the log-sum-exp with the maximum taken first and the sum in ascending
 * q; the gaussian family uses no quadrature.  elpd[k] = sum_{n < n_k} lpd[k, n], summed in row order by one thread, so its bits
 * depend on (M, D) and the problem's own data only.  Outputs: eta_mean, eta_var, pmean (K x M each, required), lpd (K x M) and
 * elpd (K): both required with y, both NULL without it.  Rows n >= n_k are never loaded and all their outputs are NaN.  A row whose
 * m or v is not finite has NaN outputs and makes elpd[k] NaN; nothing outside slice k is touched.  Everything else is what IEEE
 * arithmetic gives from the formulas (a poisson node whose e^eta overflows contributes -inf to the LSE).  The product A cov runs
 * on the fp64 MFMA over tiles of 32 rows.  1 <= D <= 64, M >= 1, K with the grid limits of the batched GSM above.  Shapes, NULL
 * arrays and overlaps (the five outputs are the written arrays) are checked before the context is looked at (then a NULL ctx);
 * every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is used.  Sets
 * GSMVI_PATH_BATCHED_PREDICT.
 */
int gsmvi_glm_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, int family, const double* A,
                                  const double* offset, const double* y, const int* counts_dev, double noise_prec,
                                  const double* noise_prec_dev, const double* mean, const double* cov, int Q, const double* gh_t,
                                  const double* gh_logw, double* eta_mean, double* eta_var, double* pmean, double* lpd,
                                  double* elpd);

/*
 * Batched Pareto-smoothed importance sampling (PSIS) diagnostic: can the fitted q_k = N(mean_k, cov_k) of K problems of one D be
 * trusted as an importance proposal for its target?  The reference's monitor (monitors.py:83-125) answers with a reverse KL up to
 * each target's unknown constant; this answers per problem on one scale (Vehtari, Simpson, Gelman, Yao, Gabry, "Pareto smoothed
 * importance sampling", JMLR 2024; tail fit: Zhang & Stephens 2009 with the weakly informative prior), with no reference twin.
 * One launch, one problem per workgroup.
 * gsmvi_psis_weights_batched_f64 runs the PSIS stage on the caller's log ratios logr (K x S); for each problem k:
 *   1. a NaN or +inf among the S ratios, or every ratio -inf: info[k] = -1 and every output of k is NaN (-inf alone is legal:
 *      a point outside the support, weight 0)
 *   2. lw = logr - max(logr);  M = ceil(min(S / 5, 3 sqrt(S)))
 *   3. sort ascending by (value, row) -- numpy's stable argsort;  cutoff = max(sorted[S - M - 1], log(DBL_MIN));  the tail is the
 *      n entries with lw > cutoff (ties at the cutoff stay out)
 *   4. n <= 4: khat = +inf, info[k] = -2, no smoothing (steps 7-8 still run)
 *   5. else x_i = exp(tail_i) - exp(cutoff) ascending, m = 30 + floor(sqrt(n)), and for j = 1 .. m
 *        b_j = (1 - sqrt(m / (j - 1/2))) / (3 x[floor(n / 4 + 1/2) - 1]) + 1 / x[n - 1]      (0-based x)
 *        kappa_j = mean_i log1p(-b_j x_i),   L_j = n (log(-b_j / kappa_j) - kappa_j - 1),   omega_j = 1 / sum_i exp(L_i - L_j)
 *      every omega_j < 10 DBL_EPSILON is dropped and the rest renormalised;  b = sum_j omega_j b_j,  kappa = mean_i log1p(-b x_i),
 *      sigma = -kappa / b,  khat = (n kappa + 5) / (n + 10)
 *   6. khat finite: the i-th smallest tail entry becomes log(sigma expm1(-khat log1p(-p_i)) / khat + exp(cutoff)), p_i = (i + 1/2) / n
 *      (khat == 0: -sigma log1p(-p_i) in place of the first term)
 *   7. lw = lw > 0 ? 0 : lw
 *   8. lse = log sum exp(lw);  lw[k] = lw - lse (K x S, in row order);  ess[k] = 1 / sum exp(2 (lw - lse));
 *      log_z[k] = lse + max(logr) - log S (the estimate of the log normalising constant);  khat[k], info[k] as above (0 = fitted)
 * khat below min(1 - 1 / log10(S), 0.7) says the proposal is usable.  Every sum is a fixed tree (a thread's entries in order, a
 * butterfly within each wave, the waves in order; no atomics), so the outputs are bit-identical from run to run.
 * gsmvi_psis_batched_f64 is the fused entry: X (K x S x D) are draws of q_k and lp (K x S) the target's values at them.  Per problem:
 *   a. R = the upper Cholesky factor of cov_k (only its upper triangle is read); a pivot that is not > 0 and finite: info[k] = 1 + that
 *      pivot and every output of k is NaN.  Else for each row R^T w = x_s - mean_k by forward substitution,
 *      logq_s = -|w|^2 / 2 - sum_i log R_ii - D / 2 log 2 pi, and logr[k, s] = lp_s - logq_s (K x S, written as computed even where
 *      step 1 then refuses them: the caller sees which row was not finite)
 *   b. the PSIS stage above on logr[k]
 *   c. with mean_is (K x D) and cov_is (K x D x D) -- both or neither --, w_s = exp(lw_s) and d_s = x_s - mean_k:
 *      mean_is[k] = mean_k + sum_s w_s d_s,  cov_is[k] = sum_s w_s d_s d_s^T - (sum_s w_s d_s)(sum_s w_s d_s)^T, exactly symmetric;
 *      each entry is summed in row order by one thread (a second read of X_k)
 * 5 <= S <= 4096, 1 <= D <= 64, K >= 1 with the grid limit of one problem per workgroup (K <= 2^24 - 1).  Shapes, NULL arrays and
 * overlaps (every output is a written array) are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is used; one capturable launch with no
 * host synchronisation.  Both set GSMVI_PATH_BATCHED_PSIS.
 */
int gsmvi_psis_weights_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int64_t S, const double* logr, double* lw,
                                   double* khat, double* ess, double* log_z, int* info);
int gsmvi_psis_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t S, const double* mean, const double* cov,
                           const double* X, const double* lp, double* logr, double* lw, double* khat, double* ess,
                           double* log_z, double* mean_is, double* cov_is, int* info);

/*
 * Batched PSIS leave-one-out (PSIS-LOO): the pointwise leave-one-out log predictive density of every observation of K fitted GLM
 * posteriors, from S draws of the approximation q_k (Vehtari, Gelman, Gabry, "Practical Bayesian model evaluation using
 * leave-one-out cross-validation and WAIC", 2017; the ratios carry the correction for draws taken from an approximation in place of
 * the posterior: Magnusson, Andersen, Jonasson, Vehtari, "Bayesian leave-one-out cross-validation for large data", 2019).  The
 * reference has no twin.  One launch, one workgroup per (problem, tile of gsmvi_psis_loo_tile(D, S) observations).
 * The model's arguments are those of gsmvi_glm_predict_batched_f64 (family, A (K x N x D), y (K x N, required), offset (K x N or
 * NULL), counts_dev (K ints or NULL), noise_prec / noise_prec_dev: the gaussian family's alone) with no prior.  X (K x S x D) are the
 * draws x_s of q_k, logr (K x S) the ratios lp - log q and lw (K x S) the normalised smoothed log weights that
 * gsmvi_psis_batched_f64 writes for the same draws.  n_k = counts_dev[k] clamped to 0 .. N (N without counts_dev).  For problem k
 * and row i < n_k:
 *   eta_si = a_i . x_s + offset_i
 *   l_si   = log p(y_i | eta_si), normalised as the lpd of gsmvi_glm_predict_batched_f64 is: t of gsmvi_glm_batched_f64's link at
 *            (eta_si, y_i, tau_k); the poisson family subtracts lgamma(y_i + 1), the gaussian family adds log(tau_k / (2 pi)) / 2;
 *            a draw that the link flags (poisson: e^eta not finite) has l_si = NaN
 *   rho_si = logr_s - l_si (one subtraction): the log ratio of the posterior without observation i to q_k, up to a constant
 *   the PSIS stage, steps 1-8 of gsmvi_psis_weights_batched_f64 above exactly (the (value, row) order of the sort and the -1 / -2
 *   verdicts included), on rho_.i gives the normalised smoothed log weights w_si, khat[k, i], ess[k, i] and info[k, i]
 *   elpd[k, i] = log sum_s exp(w_si + l_si):  the leave-one-out log predictive density
 *   lpd[k, i]  = log sum_s exp(lw_s + l_si):  the importance-corrected in-sample density; p_loo is lpd - elpd
 * both as max + log sum exp(. - max), the maximum and the sum each a fixed tree over the S draws (a thread's entries in order, a
 * butterfly within each wave, the waves in order; no atomics): the outputs are bit-identical from run to run.
 * info[k, i] = -1 (a NaN or +inf among rho_.i -- a NaN l_si, a NaN logr of a failed problem-level run --, or every rho -inf): elpd,
 * lpd, khat and ess of (k, i) are NaN.  info[k, i] = -2 (fewer than five tail entries): plain self-normalised weights and
 * khat = +inf, as in the weights entry.  Rows i >= n_k are never loaded: elpd, lpd, khat and ess are NaN and info[k, i] = -3.  A verdict
 * touches only its own (k, i).  loglik (K x N x S, or NULL) receives l_si (NaN for rows i >= n_k).  Outputs: elpd, lpd, khat, ess
 * (K x N doubles each) and info (K x N ints), all required.
 * gsmvi_psis_loo_tile(D, S) is a pure function (no GPU): the observations per workgroup, the largest count of at most 4 whose
 * l_si (S doubles each) fit in the workgroup's 160 KB of LDS beside max(stage, tiles) doubles, where stage = S2 + S + 508 + S2 / 2
 * (S2 = S rounded up to a power of two, at least 8) and tiles = 80 (16 ceil(D / 16) + 1) + 48; 0 for D or S out of bounds.
 * 1 <= D <= 64, 5 <= S <= 4096, N >= 1, K >= 1 with K ceil(N / gsmvi_psis_loo_tile(D, S)) <= 2^24 - 1.  Shapes, NULL arrays and
 * overlaps (every output is a written array) are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is used; one capturable launch with no
 * host synchronisation.  Sets GSMVI_PATH_BATCHED_LOO.
 */
int gsmvi_psis_loo_tile(int D, int64_t S);
int gsmvi_psis_loo_batched_f64(gsmvi_ctx* ctx, void* stream, int family, int64_t K, int64_t N, int D, int64_t S, const double* A,
                               const double* y, const double* offset, const int* counts_dev, double noise_prec,
                               const double* noise_prec_dev, const double* X, const double* logr, const double* lw,
                               double* loglik, double* elpd, double* lpd, double* khat, double* ess, int* info);

/*
 * Batched softmax PSIS leave-one-out: the same for K fitted multinomial logit posteriors (the model of gsmvi_softmax_batched_f64).
 * The reference has no twin.  One launch, one workgroup per (problem, tile of gsmvi_psis_loo_softmax_tile(C, P, S) observations).
 * Problem k has A_k (N x P; A is K x N x P), integer labels y_ki (K x N ints), n_k = counts_dev[k] clamped to 0 .. N valid rows (N
 * without counts_dev), C classes with D = (C - 1) P <= 64, class C - 1 the reference class, and the draws x_s (s < S; X is
 * K x S x D) of q_k, class-major as in the target: x_s[c P + j] = W_cj.  logr (K x S) and lw (K x S) are what
 * gsmvi_psis_batched_f64 writes for the same draws.  For a valid row i < n_k:
 *   eta_sic = a_i . x_s[c P .. c P + P - 1]  (c < C - 1),   eta_si,C-1 = 0
 *   m_si    = max_c eta_sic   (all C values, the 0 included)
 *   z_si    = sum_{c = 0 .. C-1} exp(eta_sic - m_si)   (class order, the reference class last)
 *   l_si    = eta_si,y_i - m_si - log z_si
 * the target's per-row density term, with no prior.  l_si is NaN in three cases: one of the C - 1 dot products is not finite; x_s
 * has a non-finite entry; y_i is outside 0 .. C - 1 (a label is only compared, never used as an index).  Nothing else produces a
 * NaN: where the product runs over zero-padded positions of a_i, the matching operand is 0 as well.
 * From there on the text is that of gsmvi_psis_loo_batched_f64 above, word for word:
 *   rho_si = logr_s - l_si (one subtraction)
 *   the PSIS stage, steps 1-8 of gsmvi_psis_weights_batched_f64 exactly (the (value, row) order of the sort and the -1 / -2
 *   verdicts included), on rho_.i gives the normalised smoothed log weights w_si, khat[k, i], ess[k, i] and info[k, i]
 *   elpd[k, i] = log sum_s exp(w_si + l_si)
 *   lpd[k, i]  = log sum_s exp(lw_s + l_si)
 * both as max + log sum exp(. - max), the maximum and the sum each a fixed tree over the S draws (a thread's entries in order, a
 * butterfly within each wave, the waves in order; no atomics): the outputs are bit-identical from run to run.
 * info[k, i] = -1 (a NaN or +inf among rho_.i, or every rho -inf): elpd, lpd, khat and ess of (k, i) are NaN.  info[k, i] = -2 (fewer
 * than five tail entries): plain self-normalised weights and khat = +inf.  Rows i >= n_k are never loaded: elpd, lpd, khat and ess
 * are NaN and info[k, i] = -3.  A verdict touches only its own (k, i).  loglik (K x N x S, or NULL) receives l_si (NaN for rows
 * i >= n_k).  Outputs: elpd, lpd, khat, ess (K x N doubles each) and info (K x N ints), all required.
 * gsmvi_psis_loo_softmax_tile(C, P, S) is a pure function (no GPU): the observations per workgroup, the largest count of at most 4
 * whose l_si (S doubles each) fit in the workgroup's 160 KB of LDS (20480 doubles) beside max(stage, tiles) doubles, where stage =
 * S2 + S + 508 + S2 / 2 (S2 = S rounded up to a power of two, at least 8) and tiles = 64 (D | 1) + 16 (4 ceil(P / 4) + 1) + 16;
 * 0 for (C, P) or S out of bounds.
 * C >= 2, P >= 1, D = (C - 1) P <= 64, 5 <= S <= 4096, N >= 1, K >= 1 with K ceil(N / gsmvi_psis_loo_softmax_tile(C, P, S)) <=
 * 2^24 - 1, K N S doubles addressable.  Shapes, NULL arrays and overlaps (loglik, elpd, lpd, khat, ess and info are the written
 * arrays, everything else is read) are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is used; one capturable launch with no
 * host synchronisation and no atomics.  Sets GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_SOFTMAX: after a reset exactly that pair
 * identifies this launch (the GLM leave-one-out sets the first bit alone, the softmax score launch the second alone).
 */
int gsmvi_psis_loo_softmax_tile(int C, int P, int64_t S);
int gsmvi_psis_loo_softmax_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t N, int64_t S,
                                       const double* A, const int* labels, const int* counts_dev, const double* X,
                                       const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                       double* khat, double* ess, int* info);

/*
 * Batched negative binomial PSIS leave-one-out: the same for K fitted posteriors of the overdispersed count model of
 * gsmvi_negbin_batched_f64, whose draws carry a shape parameter.  The reference has no twin.  One launch, one workgroup per
 * (problem, tile of gsmvi_psis_loo_negbin_tile(P, S) observations).
 * Problem k has A_k (N x P; A is K x N x P), responses y_ki >= 0 (K x N), an optional offset o_ki (K x N, or NULL), n_k =
 * counts_dev[k] clamped to 0 .. N valid rows (N without counts_dev), and the draws x_s = (beta_s, theta_s) (s < S; X is K x S x D,
 * D = P + 1 <= 64, theta = log r the log of the size) of q_k.  logr (K x S) and lw (K x S) are what gsmvi_psis_batched_f64 writes
 * for the same draws.  For a valid row i < n_k:
 *   eta_si = a_i . beta_s + o_i
 *   l_si   = t(eta_si, theta_s, y_i) - lgamma(y_i + 1)
 * with t the per-row density term of gsmvi_negbin_batched_f64 (lgamma(y + r) - lgamma(r) - r softplus(eta - theta) - y softplus(theta
 * - eta), r = e^theta; the lgamma difference is formed as a difference, never from two lgamma calls, and e^eta is never formed).  The
 * term -lgamma(y_i + 1) is INCLUDED, so l_si is the normalised log probability of the count y_i -- as the poisson family of
 * gsmvi_psis_loo_batched_f64 includes it: the elpd of the two launches are on one scale and may be subtracted (is the shape
 * parameter worth having over Poisson?).  No prior enters.
 * A draw is flagged when one of its D entries, theta included, is not finite, or when e^theta is not a positive normal number
 * (|theta| above about 708: the row flag of gsmvi_negbin_batched_f64); a flagged draw has l_si = NaN for every observation of the
 * problem.  The flag is taken from the draw's entries, not from the product: nothing else produces a NaN.
 * From there on the text is that of gsmvi_psis_loo_batched_f64 above, word for word:
 *   rho_si = logr_s - l_si (one subtraction)
 *   the PSIS stage, steps 1-8 of gsmvi_psis_weights_batched_f64 exactly (the (value, row) order of the sort and the -1 / -2
 *   verdicts included), on rho_.i gives the normalised smoothed log weights w_si, khat[k, i], ess[k, i] and info[k, i]
 *   elpd[k, i] = log sum_s exp(w_si + l_si)
 *   lpd[k, i]  = log sum_s exp(lw_s + l_si)
 * both as max + log sum exp(. - max), the maximum and the sum each a fixed tree over the S draws (a thread's entries in order, a
 * butterfly within each wave, the waves in order; no atomics): the outputs are bit-identical from run to run.
 * info[k, i] = -1 (a NaN or +inf among rho_.i -- a flagged draw, a NaN logr --, or every rho -inf): elpd, lpd, khat and ess of (k, i)
 * are NaN.  info[k, i] = -2 (fewer than five tail entries): plain self-normalised weights and khat = +inf.  Rows i >= n_k are never
 * loaded: elpd, lpd, khat and ess are NaN and info[k, i] = -3.  A verdict touches only its own (k, i).  loglik (K x N x S, or NULL)
 * receives l_si (NaN for rows i >= n_k).  Outputs: elpd, lpd, khat, ess (K x N doubles each) and info (K x N ints), all required.
 * gsmvi_psis_loo_negbin_tile(P, S) is a pure function (no GPU): the observations per workgroup, the largest count of at most 4
 * whose l_si (S doubles each) fit in the workgroup's 160 KB of LDS (20480 doubles) beside max(stage, tiles) doubles, where stage =
 * S2 + S + 508 + S2 / 2 (S2 = S rounded up to a power of two, at least 8) and tiles = 80 (4 ceil(P / 4) + 1) + 240; 0 for P or S
 * out of bounds.
 * P >= 1, D = P + 1 <= 64, 5 <= S <= 4096, N >= 1, K >= 1 with K ceil(N / gsmvi_psis_loo_negbin_tile(P, S)) <= 2^24 - 1, K N S
 * doubles addressable.  Shapes, NULL arrays and overlaps (loglik, elpd, lpd, khat, ess and info are the written arrays, everything
 * else is read) are checked before the context is looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before
 * anything is enqueued.  Inputs are only read; no context workspace is used; one capturable launch with no host synchronisation
 * and no atomics.  Sets GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET: after a reset exactly that pair identifies this launch
 * or its ordinal sibling below (the GLM leave-one-out sets the first bit alone, the negative binomial score launch the second alone).
 */
int gsmvi_psis_loo_negbin_tile(int P, int64_t S);
int gsmvi_psis_loo_negbin_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t N, int64_t S, const double* A,
                                      const double* y, const double* offset, const int* counts_dev, const double* X,
                                      const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                      double* khat, double* ess, int* info);

/*
 * Batched ordinal PSIS leave-one-out: the same for K fitted posteriors of the cumulative-logit (proportional odds) model of
 * gsmvi_ordinal_batched_f64, whose draws carry the C - 1 cutpoint parameters behind the coefficients.  The reference has no twin.
 * One launch, one workgroup per (problem, tile of gsmvi_psis_loo_ordinal_tile(P, C, S) observations).
 * Problem k has A_k (N x P, no intercept column; A is K x N x P), labels y_ki in 0 .. C - 1 (K x N ints; a label outside the range
 * is clamped into it), an optional offset o_ki (K x N, or NULL), n_k = counts_dev[k] clamped to 0 .. N valid rows (N without
 * counts_dev), and the draws x_s = (beta_s, delta_s) (s < S; X is K x S x D, D = P + C - 1 <= 64) of q_k.  logr (K x S) and lw
 * (K x S) are what gsmvi_psis_batched_f64 writes for the same draws.  For a draw s and a valid row i < n_k:
 *   cut_s0 = delta_s0,   cut_sj = cut_s,j-1 + e^{delta_sj}  (j = 1 .. C - 2, one chain in ascending j: the score launch's bits)
 *   eta_si = a_i . beta_s + o_i
 *   l_si   = t(eta_si, cut_s, e^{delta_s}, y_i) = log P(y_i | eta_si, cut_s)
 * with t the per-row density term of gsmvi_ordinal_batched_f64: with a = cut_{y-1} - eta (y >= 1), b = cut_y - eta (y <= C - 2) and
 * w = e^{delta_y} for an interior label, t = -[y <= C - 2] softplus(-b) - [y >= 1] softplus(a) + [interior] log(1 - e^{-w}); no two
 * probabilities are subtracted and e^{+|z|} is never formed.  The categorical probability is normalised: no constant is added, and
 * elpd is on the scale of gsmvi_psis_loo_softmax_batched_f64 on the same labels (does proportional odds beat a multinomial
 * logit?).  No prior enters.
 * A draw is flagged when one of its D entries is not finite, or when some e^{delta_j}, j >= 1, is not a positive normal number
 * (|delta_j| above about 708: the row flag of gsmvi_ordinal_batched_f64), whether or not a row is labelled j; a flagged draw has
 * l_si = NaN for every observation of the problem.  The flag is taken from the draw's entries, not from the product: nothing else
 * produces a NaN.
 * From there on the text is that of gsmvi_psis_loo_batched_f64 above, word for word:
 *   rho_si = logr_s - l_si (one subtraction)
 *   the PSIS stage, steps 1-8 of gsmvi_psis_weights_batched_f64 exactly (the (value, row) order of the sort and the -1 / -2
 *   verdicts included), on rho_.i gives the normalised smoothed log weights w_si, khat[k, i], ess[k, i] and info[k, i]
 *   elpd[k, i] = log sum_s exp(w_si + l_si)
 *   lpd[k, i]  = log sum_s exp(lw_s + l_si)
 * both as max + log sum exp(. - max), the maximum and the sum each a fixed tree over the S draws (a thread's entries in order, a
 * butterfly within each wave, the waves in order; no atomics): the outputs are bit-identical from run to run.
 * info[k, i] = -1 (a NaN or +inf among rho_.i -- a flagged draw, a NaN logr --, or every rho -inf): elpd, lpd, khat and ess of (k, i)
 * are NaN.  info[k, i] = -2 (fewer than five tail entries): plain self-normalised weights and khat = +inf.  Rows i >= n_k are never
 * loaded: elpd, lpd, khat and ess are NaN and info[k, i] = -3.  A verdict touches only its own (k, i).  loglik (K x N x S, or NULL)
 * receives l_si (NaN for rows i >= n_k).  Outputs: elpd, lpd, khat, ess (K x N doubles each) and info (K x N ints), all required.
 * gsmvi_psis_loo_ordinal_tile(P, C, S) is a pure function (no GPU): the observations per workgroup, the largest count of at most 4
 * whose l_si (S doubles each) fit in the workgroup's 160 KB of LDS (20480 doubles) beside max(stage, tiles) doubles, where stage =
 * S2 + S + 508 + S2 / 2 (S2 = S rounded up to a power of two, at least 8) and tiles = 80 (4 ceil(P / 4) + 1) + 64 ((C - 1) | 1) +
 * 344 (at most 5736, at (P, C) = (61, 4): 4 for every legal shape at S <= 2048, 2 at S = 4096); 0 for P, C or S out of bounds.
 * 2 <= C <= 64, 1 <= P <= 65 - C, 5 <= S <= 4096, N >= 1, K >= 1 with K ceil(N / gsmvi_psis_loo_ordinal_tile(P, C, S)) <= 2^24 - 1,
 * K N S doubles addressable.  Shapes, NULL arrays and overlaps (loglik, elpd, lpd, khat, ess and info are the written arrays,
 * everything else is read) are checked before the context is looked at (then a NULL ctx); every failure returns
 * GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no context workspace is used; one capturable launch with
 * no host synchronisation and no atomics.  Sets GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET, the pair of the negative
 * binomial leave-one-out above (all 32 bits are taken): after a reset the pair says that one of the two ran (the GLM
 * leave-one-out sets the first bit alone, the ordinal score launch the second alone).
 */
int gsmvi_psis_loo_ordinal_tile(int P, int C, int64_t S);
int gsmvi_psis_loo_ordinal_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t N, int64_t S, const double* A,
                                       const int* y, const double* offset, const int* counts_dev, const double* X,
                                       const double* logr, const double* lw, double* loglik, double* elpd, double* lpd,
                                       double* khat, double* ess, int* info);

/*
 * Shared-design PSIS leave-one-out: the same for K fitted posteriors of the model of gsmvi_glm_shared_batched_f64: K GLMs on ONE
 * design matrix with observation weights.  The reference has no twin.  One launch, one workgroup per (problem, tile of
 * gsmvi_psis_loo_tile(D, S) consecutive observations), k-major; A is never replicated.
 * A (N x D) is the one design matrix with rows a_i.  Problem k has responses y_ki (K x N, required), an optional offset o_ki (K x N, or
 * NULL), observation weights v_ki >= 0 (K x N, or NULL: every v = 1), the noise precision tau_k (noise_prec / noise_prec_dev: the
 * gaussian family's alone) and no prior.  X (K x S x D) are the draws x_s of q_k; logr (K x S) and lw (K x S) are what
 * gsmvi_psis_batched_f64 writes for the same draws, logr from the WEIGHTED density lp_k(x) = sum_i v_ki t_ki(x) - lam_k |x|^2 / 2.
 * Row i of problem k is valid iff v_ki > 0: the selection of gsmvi_glm_shared_hessian_batched_f64.  A weight of 0 or NaN removes
 * the row whatever y and the offset hold there (they are never fed to the link); the valid rows are an arbitrary subset, not a
 * prefix.  For a valid row:
 *   eta_si = a_i . x_s + o_ki
 *   l_si   = the log density of ONE unit observation, UNWEIGHTED: l_si of gsmvi_psis_loo_batched_f64 exactly (the poisson family
 *            subtracts lgamma(y + 1), the gaussian family adds log(tau_k / (2 pi)) / 2; a flagged draw has l_si = NaN)
 *   rho_si = logr_s - v_ki l_si (one product, one subtraction, not fused): leaving row i out removes its whole weighted term.  With
 *            v_ki = 1 the product is exact and rho has the bits of gsmvi_psis_loo_batched_f64
 * From there on the text is that of gsmvi_psis_loo_batched_f64 above, word for word:
 *   the PSIS stage, steps 1-8 of gsmvi_psis_weights_batched_f64 exactly (the (value, row) order of the sort and the -1 / -2
 *   verdicts included), on rho_.i gives the normalised smoothed log weights w_si, khat[k, i], ess[k, i] and info[k, i]
 *   elpd[k, i] = log sum_s exp(w_si + l_si):  the leave-one-out log predictive density of one unit observation at row i
 *   lpd[k, i]  = log sum_s exp(lw_s + l_si)
 * both as max + log sum exp(. - max), the maximum and the sum each a fixed tree over the S draws: the outputs are bit-identical from
 * run to run.  info[k, i] = -1 (a NaN or +inf among rho_.i, or every rho -inf): elpd, lpd, khat and ess of (k, i) are NaN.
 * info[k, i] = -2 (fewer than five tail entries): plain self-normalised weights and khat = +inf.  A row that is not valid has NaN in
 * elpd, lpd, khat and ess and info[k, i] = -3; it flags nothing else.  A verdict touches only its own (k, i).  loglik (K x N x S, or
 * NULL) receives l_si (NaN for the rows that are not valid).  Outputs: elpd, lpd, khat, ess (K x N doubles each) and info (K x N
 * ints), all required.  The per-problem sums are the caller's: with c_i = v_ki elpd[k, i] over the n_k valid rows, elpd_loo = sum
 * c_i, p_loo = sum v_ki (lpd - elpd), se = sqrt(n_k var(c_i)).  A row of weight 0 is NOT scored as a held-out row.
 * With weights NULL or all 1 every output has the bits of gsmvi_psis_loo_batched_f64 on K copies of A; with 0 / 1 weights that form
 * a prefix, those of its counts_dev.
 * 1 <= D <= 64, 5 <= S <= 4096, N >= 1, K >= 1 with K ceil(N / gsmvi_psis_loo_tile(D, S)) <= 2^24 - 1, K N S doubles addressable.
 * Shapes, NULL arrays and overlaps (loglik, elpd, lpd, khat, ess and info are the written arrays, everything else is read; A counts
 * N D doubles) are checked before the context is looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before
 * anything is enqueued.  Inputs are only read; no context workspace is used; one capturable launch with no host synchronisation
 * and no atomics.  Sets GSMVI_PATH_BATCHED_LOO | GSMVI_PATH_BATCHED_TARGET (no bit of its own).
 */
int gsmvi_psis_loo_shared_batched_f64(gsmvi_ctx* ctx, void* stream, int family, int64_t K, int64_t N, int D, int64_t S,
                                      const double* A, const double* y, const double* offset, const double* weights,
                                      double noise_prec, const double* noise_prec_dev, const double* X, const double* logr,
                                      const double* lw, double* loglik, double* elpd, double* lpd, double* khat, double* ess,
                                      int* info);

/*
 * Batched softmax posterior predictive: what the fitted q_k = N(mean_k, cov_k) of K multinomial logit regressions (the model of
 * gsmvi_softmax_batched_f64) says about M new rows per problem, from S draws of q_k: the class probabilities and, with the rows'
 * labels, the log predictive density of every row (the held-out score).  The C - 1 linear predictors of a row are coupled, so the
 * one-dimensional quadrature of gsmvi_glm_predict_batched_f64 does not apply; the draws are those of gsmvi_kl_draw_batched_f64,
 * optionally with the smoothed weights of gsmvi_psis_batched_f64.  The reference has no twin.  One launch, one 256-thread workgroup
 * per (problem, tile of 16 new rows).
 * A (K x M x P) are the new rows, labels (K x M ints, or NULL) their classes, n_k = counts_dev[k] clamped to 0 .. M valid rows (M
 * without counts_dev), C classes with D = (C - 1) P <= 64, class C - 1 the reference class, X (K x S x D) the draws x_s of q_k,
 * class-major as in the target: x_s[c P + j] = W_cj.  lw (K x S, or NULL) are normalised log weights, e.g. the log_weights of
 * gsmvi_psis_batched_f64 for the same draws; NULL means uniform: lw_s = -log S and w_s = 1.0 / S.  For a valid row i < n_k and draw s:
 *   eta_sic = a_i . x_s[c P .. c P + P - 1]  (c < C - 1),   eta_si,C-1 = 0
 *   m_si    = max_c eta_sic   (all C values, the 0 included)
 *   z_si    = sum_{c = 0 .. C-1} exp(eta_sic - m_si)   (class order, the reference class last)
 *   p_sic   = exp(eta_sic - m_si) / z_si
 *   prob[k, i, c] = sum_s w_s p_sic,   w_s = exp(lw_s)
 *   l_si    = eta_si,y_i - m_si - log z_si
 *   lpd[k, i]     = log sum_s exp(lw_s + l_si)
 * lpd is a log-sum-exp that cannot underflow: a fixed tree of (max, scaled sum) pairs merged as (m1, s1) + (m2, s2) =
 * (M, s1 e^(m1 - M) + s2 e^(m2 - M)), M = max(m1, m2); a pair whose maximum is -inf contributes 0.  A held-out row whose true
 * class has eta near -800 at every draw keeps a finite lpd (the log of a linear-space sum would be -inf).  prob is summed in linear
 * space.  Every sum is a fixed tree (a lane's entries in order, a fixed cross-lane order, the draw tiles in order, the waves in
 * order; no atomics): the outputs are bit-identical from run to run.
 * Draws s >= S of a partial tile contribute nothing (masked, not weighted).  A draw whose eta is not finite for row i (a non-finite
 * entry of a_i or of x_s, 0 x inf included; where the product runs over zero-padded positions of a_i the matching operand is 0 as
 * well, so nothing else does it) makes the C probabilities and the lpd of row i NaN.  A problem whose lw holds a NaN or +inf, or
 * only -inf, has NaN in every valid row (a lone -inf is legal: weight 0).  A label outside 0 .. C - 1 gives a NaN lpd for its row
 * only (a label is only compared, never used as an index).  Rows i >= n_k are never loaded and their outputs are NaN.  A verdict
 * touches only its own (k, i) or k.  Outputs: prob (K x M x C, required) and lpd (K x M): required exactly when labels is given,
 * NULL otherwise.
 * gsmvi_softmax_predict_lds_bytes(C, P) is a pure function (no GPU): the dynamic LDS of the launch in bytes, 8 (64 (D | 1) +
 * 16 (4 ceil(P / 4) + 1) + 64 C + 344) -- the tile of 64 draws, the 16 rows, the accumulators of (wave, class, row), the weights
 * of the tile and the waves' partial results --, at most 69952 (C = 65, P = 1), inside the workgroup's 160 KB; 0 for (C, P) out of
 * bounds.
 * C >= 2, P >= 1, D = (C - 1) P <= 64, 1 <= S <= 4096, M >= 1, K >= 1 with K ceil(M / 16) <= 2^24 - 1.  Shapes, NULL arrays, the
 * labels / lpd pairing and overlaps (prob and lpd are the written arrays, everything else is read) are checked before the context
 * is looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no
 * context workspace is used; one capturable launch with no host synchronisation and no atomics.  Sets GSMVI_PATH_BATCHED_PREDICT |
 * GSMVI_PATH_BATCHED_SOFTMAX: after a reset exactly that pair identifies this launch (the GLM predictive sets the first bit alone,
 * the softmax score launch the second alone).
 */
int gsmvi_softmax_predict_lds_bytes(int C, int P);
int gsmvi_softmax_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int C, int P, int64_t M, int64_t S,
                                      const double* A, const int* labels, const int* counts_dev, const double* X,
                                      const double* lw, double* prob, double* lpd);

/*
 * Batched negative binomial posterior predictive: what the fitted q_k = N(mean_k, cov_k) of K overdispersed count regressions (the
 * model of gsmvi_negbin_batched_f64) says about M new rows per problem, from S draws of q_k: three log moments of the predictive
 * count and, with the rows' counts, the log predictive density of every row (the held-out score, on the scale of
 * gsmvi_psis_loo_negbin_batched_f64).  theta = log r is a coordinate of q_k and is correlated with beta, so a row's density depends
 * on the pair (eta, theta) and the one-dimensional quadrature of gsmvi_glm_predict_batched_f64 does not apply; the draws are those
 * of gsmvi_kl_draw_batched_f64, optionally with the smoothed weights of gsmvi_psis_batched_f64.  The reference has no twin.  One
 * launch, one 256-thread workgroup per (problem, tile of 16 new rows).
 * A (K x M x P) are the new rows, y (K x M, or NULL) their counts >= 0, offset (K x M, or NULL) is added to the linear predictor,
 * n_k = counts_dev[k] clamped to 0 .. M valid rows (M without counts_dev), X (K x S x D, D = P + 1 <= 64) the draws x_s = (beta_s,
 * theta_s) of q_k.  lw (K x S, or NULL) are normalised log weights, e.g. the log_weights of gsmvi_psis_batched_f64 for the same
 * draws; NULL means uniform: lw_s = -log S.  For a valid row i < n_k and draw s:
 *   eta_si = a_i . beta_s + o_i,   theta_s = x_s[P],   r_s = e^theta_s
 *   lmom[k, i, 0] = log sum_s exp(lw_s + eta_si)                 (log E[mu])
 *   lmom[k, i, 1] = log sum_s exp(lw_s + 2 eta_si)               (log E[mu^2])
 *   lmom[k, i, 2] = log sum_s exp(lw_s + 2 eta_si - theta_s)     (log E[mu^2 / r])
 *   l_si   = t(eta_si, theta_s, y_i) - lgamma(y_i + 1)
 *   lpd[k, i]     = log sum_s exp(lw_s + l_si)
 * with t the per-row density term of gsmvi_negbin_batched_f64 at the same eta (the same device function, whole).  The predictive
 * mean is e^lmom0 and the predictive variance E[mu + mu^2 / r] + Var[mu] = e^lmom0 + e^lmom2 + e^lmom1 - e^(2 lmom0); they are left
 * to the caller because e^lmom0 overflows above 709.78 where the logs do not.  The term -lgamma(y_i + 1) is INCLUDED, as in
 * gsmvi_psis_loo_negbin_batched_f64.  Without y the density is not evaluated.
 * All four are log-sum-exps that cannot overflow or underflow where the truth is finite: a fixed tree of (max, scaled sum) pairs
 * merged as (m1, s1) + (m2, s2) = (M, s1 e^(m1 - M) + s2 e^(m2 - M)), M = max(m1, m2); a pair whose maximum is -inf contributes 0;
 * e^eta is never formed.  Every sum is a fixed tree or chain (a lane's entries in order, a fixed cross-lane order, the draw tiles
 * in order, the waves in order; no atomics): the outputs are bit-identical from run to run.
 * Draws s >= S of a partial tile contribute nothing (masked, not weighted).  A draw s < S is flagged when one of its D entries,
 * theta included, is not finite, or when e^theta is not a positive normal number (|theta| above about 708: the row flag of
 * gsmvi_negbin_batched_f64); the flag is taken from the draw's entries, not from the product, and a flagged draw makes every valid
 * row of its problem NaN whatever its weight.  A non-finite eta_si at a draw s < S (a non-finite entry of a_i or o_i) makes the
 * outputs of row i NaN.  A problem whose lw holds a NaN or +inf, or only -inf, has NaN in every valid row (a lone -inf is legal:
 * weight 0).  Rows i >= n_k are never loaded and their outputs are NaN.  A verdict touches only its own (k, i) or k.  Outputs:
 * lmom (K x M x 3, required) and lpd (K x M): required exactly when y is given, NULL otherwise.
 * The launch asks for 8 (80 (4 ceil(P / 4) + 1) + 824) bytes of dynamic LDS, at most 48192 (P = 63).
 * P >= 1, D = P + 1 <= 64, 1 <= S <= 4096, M >= 1, 1 <= K <= 2^24 - 1 with K ceil(M / 16) <= 2^24 - 1.  Shapes, NULL arrays, the
 * y / lpd pairing and overlaps (lmom and lpd are the written arrays, everything else is read) are checked before the context is
 * looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no
 * context workspace is used; one capturable launch with no host synchronisation and no atomics.  Sets GSMVI_PATH_BATCHED_PREDICT |
 * GSMVI_PATH_BATCHED_TARGET: after a reset exactly that pair identifies this launch or gsmvi_glm_shared_predict_batched_f64's
 * (the GLM predictive sets the first bit alone, the negative binomial score launch the second alone).
 */
int gsmvi_negbin_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int64_t M, int64_t S, const double* A,
                                     const double* y, const double* offset, const int* counts_dev, const double* X,
                                     const double* lw, double* lmom, double* lpd);

/*
 * Batched ordinal posterior predictive: what the fitted q_k = N(mean_k, cov_k) of K cumulative-logit (proportional odds) regressions
 * (the model of gsmvi_ordinal_batched_f64) says about M new rows per problem, from S draws of q_k: the class probabilities and, with
 * the rows' labels, the log predictive density of every row (the held-out score, on the scale of the lpd of
 * gsmvi_psis_loo_ordinal_batched_f64).  The cutpoints are coordinates of q_k and are correlated with beta, so a row's probabilities
 * depend on the whole draw and the one-dimensional quadrature of gsmvi_glm_predict_batched_f64 does not apply; the draws are those
 * of gsmvi_kl_draw_batched_f64, optionally with the smoothed weights of gsmvi_psis_batched_f64.  The reference has no twin.  One
 * launch, one 256-thread workgroup per (problem, tile of 16 new rows); no (K, S, M, C) block is formed.
 * A (K x M x P) are the new rows, y (K x M ints, or NULL) their labels in 0 .. C - 1, offset (K x M, or NULL) is added to the linear
 * predictor, n_k = counts_dev[k] clamped to 0 .. M valid rows (M without counts_dev), C classes with D = P + C - 1 <= 64, X
 * (K x S x D) the draws x_s = (beta_s, delta_s) of q_k, beta first.  lw (K x S, or NULL) are normalised log weights, e.g. the
 * log_weights of gsmvi_psis_batched_f64 for the same draws; NULL means uniform: lw_s = -log S and w_s = 1.0 / S.  For a valid row
 * i < n_k and draw s:
 *   cut_s0 = delta_s0,  cut_sj = cut_s,j-1 + w_sj,  w_sj = exp(delta_sj)   (j = 1 .. C - 2: one chain in ascending j, the bits of
 *                                                                          gsmvi_ordinal_batched_f64's prologue)
 *   eta_si = a_i . beta_s + o_i
 *   z_sij  = cut_sj - eta_si
 *   p_si0  = sigma(z_si0),   p_si,C-1 = sigma(-z_si,C-2),   p_sic = sigma(z_sic) sigma(-z_si,c-1) (-expm1(-w_sc))   (0 < c < C - 1)
 *   prob[k, i, c] = sum_s w_s p_sic,   w_s = exp(lw_s)
 *   l_si   = t of the link of gsmvi_ordinal_batched_f64 at the label y_i (the l_si of gsmvi_psis_loo_ordinal_batched_f64: the same
 *            device function, the same bits at the same eta and cutpoints)
 *   lpd[k, i]     = log sum_s exp(lw_s + l_si)
 * No two probabilities are subtracted: sigma(cut_c - eta) - sigma(cut_{c-1} - eta) = sigma(z_c) sigma(-z_{c-1}) (1 - e^{-w_c}), with
 * sigma(z) and sigma(-z) from one exp(-|z|) and one -expm1(-w) per (draw, interior class); at |eta| around 1000 the probabilities
 * stay finite, with exact 0 and 1 entries.  lpd is a log-sum-exp that cannot underflow: a fixed tree of (max, scaled sum) pairs
 * merged as (m1, s1) + (m2, s2) = (M, s1 e^(m1 - M) + s2 e^(m2 - M)), M = max(m1, m2); a pair whose maximum is -inf contributes 0;
 * it is never the log of a linear-space sum.  prob is summed in linear space.  Every sum is a fixed tree or chain (a lane's entries
 * in order, a fixed cross-lane order, the draw tiles in order, the waves in order; no atomics): the outputs are bit-identical from
 * run to run and a problem's bits do not depend on K or on its neighbours.
 * Draws s >= S of a partial tile contribute nothing (masked, not weighted).  A draw s < S is flagged by the rule of
 * gsmvi_psis_loo_ordinal_batched_f64: a non-finite entry of x_s, or some w_sj, j >= 1, that is not a positive normal number; the
 * flag is taken from the draw's entries, not from the product, and a flagged draw makes every valid row of its problem NaN whatever
 * its weight.  A non-finite eta_si at a draw s < S (a non-finite entry of a_i or o_i) makes the outputs of row i NaN.  A problem
 * whose lw holds a NaN or +inf, or only -inf, has NaN in every valid row (a lone -inf is legal: weight 0).  A label outside
 * 0 .. C - 1 gives a NaN lpd for its row only (a label is compared or clamped, never used as an unchecked index).  Rows i >= n_k
 * are never loaded and their outputs are NaN.  A verdict touches only its own (k, i) or k.  Outputs: prob (K x M x C, required) and
 * lpd (K x M): required exactly when y is given, NULL otherwise.
 * gsmvi_ordinal_predict_lds_bytes(P, C) is a pure function (no GPU): the dynamic LDS of the launch in bytes, 8 (80 (4 ceil(P / 4) +
 * 1) + 128 ((C - 1) | 1) + 64 C + 616) -- the tile of 64 draws' beta and the 16 rows, the tables of the cutpoints and of the gap
 * factors, the accumulators of (wave, class, row), the weights and gap cells of the tile and the waves' partial results --,
 * at most 105408 (P = 1, C = 64), inside the workgroup's 160 KB; 0 for (P, C) out of bounds.
 * 2 <= C <= 64, 1 <= P <= 65 - C, 1 <= S <= 4096, M >= 1, 1 <= K <= 2^24 - 1 with K ceil(M / 16) <= 2^24 - 1.  Shapes, NULL arrays,
 * the y / lpd pairing and overlaps (prob and lpd are the written arrays, everything else is read) are checked before the context is
 * looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG before anything is enqueued.  Inputs are only read; no
 * context workspace is used; one capturable launch with no host synchronisation and no atomics.  Sets GSMVI_PATH_BATCHED_PREDICT |
 * GSMVI_PATH_BATCHED_TARGET (no bit of its own: the pair is also gsmvi_negbin_predict_batched_f64's and
 * gsmvi_glm_shared_predict_batched_f64's).
 */
int gsmvi_ordinal_predict_lds_bytes(int P, int C);
int gsmvi_ordinal_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int P, int C, int64_t M, int64_t S, const double* A,
                                      const int* y, const double* offset, const int* counts_dev, const double* X,
                                      const double* lw, double* prob, double* lpd);

/*
 * Shared-design GLM posterior predictive: gsmvi_glm_predict_batched_f64 for K fitted posteriors q_k = N(mean_k, cov_k) on ONE
 * shared set of new rows, with per-problem row weights: the held-out score of K-fold cross-validation on the model of
 * gsmvi_glm_shared_batched_f64 (F folds x L settings are K = F L problems on one design).  The reference has no twin.  One launch;
 * A is never replicated.
 * A (M x D) is the one matrix of new rows a_m.  Problem k has mean_k (D), cov_k (D x D, read as given, both triangles), an optional
 * offset o_km (K x M, or NULL), optional responses y_km (K x M, or NULL), optional row weights v_km (K x M, or NULL: every v = 1)
 * and, for the gaussian family, the noise precision tau_k (noise_prec / noise_prec_dev); no prior.  gh_t and gh_logw (Q each) are
 * the nodes and the logarithms of the weights of the Q-point Gauss-Hermite rule (weight exp(-t^2)), 1 <= Q <= 64.
 * Row m of problem k is valid iff weights is NULL or v_km > 0: the selection of gsmvi_glm_shared_hessian_batched_f64 and
 * gsmvi_psis_loo_shared_batched_f64.  A weight of 0 or NaN removes the row; the valid rows are an arbitrary subset, not a prefix.
 * For a valid row, eta_mean[k, m], eta_var[k, m], pmean[k, m] and lpd[k, m] are what gsmvi_glm_predict_batched_f64 defines for row
 * m of a problem whose design is A: m = a_m . mean_k + o_km, v = a_m^T cov_k a_m (eta_var, the raw value), v+ = max(v, 0), the four
 * families' closed forms, the Gauss-Hermite log-sum-exp (the maximum first, then the sum of exp(. - max) in ascending q) with t and
 * r of gsmvi_glm_batched_f64's link, and the row's NaN rule (m or v not finite: the row's outputs are NaN).
 *   lpd[k, m]  = the log predictive density of ONE unit observation y_km, UNWEIGHTED: the convention of
 *                gsmvi_psis_loo_shared_batched_f64
 *   elpd[k]    = sum over the valid rows of v_km lpd[k, m] (v = 1 without weights; one product, one addition, not fused), summed
 *                by one thread in ascending m, the rows that are not valid skipped; 0 for a problem without a valid row; NaN when a
 *                valid row's lpd is
 * For a row that is not valid, y[k, m] and offset[k, m] are never read (a NaN y, an infinite offset there are harmless), the row's
 * four outputs are NaN and it adds nothing to elpd[k].  Without y, lpd and elpd are NULL; the weights still select the rows of the
 * other three outputs.  A is shared: a non-finite entry in row m of it reaches row m of every problem, and only row m; a non-finite
 * entry of mean_k or cov_k reaches problem k alone.
 * With weights NULL or all exactly 1.0 every output has the bits of gsmvi_glm_predict_batched_f64 on K copies of A; with 0 / 1
 * weights that form a prefix, those of its counts_dev.  The outputs are bit-identical from run to run and do not depend on K or on
 * the other problems of the launch.
 * 1 <= D <= 64, M >= 1, K >= 1 within the launch bound of gsmvi_glm_shared_hessian_batched_f64, K M D doubles addressable.  Shapes,
 * the family and its noise precision, Q, NULL arrays, the y / lpd / elpd pairing (lpd and elpd are required with y and only with it)
 * and overlaps (eta_mean, eta_var, pmean, lpd and elpd are the written arrays, everything else, weights included, is read; A counts
 * M D doubles) are checked before the context is looked at (then a NULL ctx); every failure returns GSMVI_ERR_BAD_ARG with its own
 * message before anything is enqueued.  Inputs are only read; no context workspace is used; one capturable launch with no host
 * synchronisation and no atomics; at most 53.5 KB of dynamic LDS.  Sets GSMVI_PATH_BATCHED_PREDICT | GSMVI_PATH_BATCHED_TARGET (no
 * bit of its own: the pair is also gsmvi_negbin_predict_batched_f64's).
 */
int gsmvi_glm_shared_predict_batched_f64(gsmvi_ctx* ctx, void* stream, int64_t K, int D, int64_t M, int family, const double* A,
                                         const double* offset, const double* y, const double* weights, double noise_prec,
                                         const double* noise_prec_dev, const double* mean, const double* cov, int Q,
                                         const double* gh_t, const double* gh_logw, double* eta_mean, double* eta_var, double* pmean,
                                         double* lpd, double* elpd);

/*
 * Upper Cholesky factor R (R^T R = S, R upper triangular, strictly-lower part zeroed) of a
 * symmetric matrix; *info_dev (device int) = 0 if S is positive definite, else 1 + index of the
 * first failing pivot (also set when a NaN is met).  Replaces np.linalg.cholesky inside
 * _check_goodness (gsm_numpy.py:132-146) and supplies the sampling factor.  R must not alias S; only the upper
 * triangle of S is read (plus the full diagonal blocks).  Two launches (a flag-clearing one and the persistent task graph
 * k_potrf_dag, round 6; ceil(D/64) launches before, still behind the knob "potrf_dag" = 0); every wait inside it is bounded:
 * *info_dev = D + 1 reports a wait that ran out of its poll budget (a shared, stalled GPU), never a hang.
 */
int gsmvi_potrf_f64(gsmvi_ctx* ctx, void* stream, int D, const double* S, int lds,
                    double* R, int ldr, int* info_dev);

/*
 * C = F^T F for a square factor F (D x D, any square factor with F^T F = cov): the covariance a factor-form fit
 * returns and hands to its monitor (the reference's fit returns cov, gsm_numpy.py:129; monitors.py:99).  C is
 * exactly symmetric.  Once per fit / per monitor checkpoint, not per iteration.
 */
int gsmvi_gram_f64(gsmvi_ctx* ctx, void* stream, int D, const double* F, int ldf, double* C, int ldc);

/*
 * C = F^T F + (shift + *shift_dev) I (shift_dev may be NULL; a device double read when the kernel executes).  The reference's
 * BaM loop adds jitter * I to the covariance after EVERY update (bam.py:198, default 1e-6); a diagonal shift is not a low-rank
 * change of a square factor, so a factor-form fit carries the shift it owes and absorbs it every few iterations by
 * re-factorising this matrix with gsmvi_potrf_f64 (gsm-vi_amd/bam.py, jitter_every).  shift_dev lets the caller count only
 * ACCEPTED updates without a host synchronisation (a reverted iteration adds no jitter in the reference, bam.py:208-212).
 */
int gsmvi_gram_shift_f64(gsmvi_ctx* ctx, void* stream, int D, const double* F, int ldf, double shift, const double* shift_dev,
                         double* C, int ldc);

/*
 * Whitened residuals Z = (X - 1 mu^T) R^-1 for nrows rows of X and an upper Cholesky factor R (R^T R = cov), and
 * (if logdiag_dev != NULL) logdiag_dev[0] = sum_i log R_ii.  Together they give the row-wise Gaussian log density
 * log N(x; mu, cov) = -1/2 |z|^2 - sum_i log R_ii - D/2 log(2 pi) that the reference's KLMonitor evaluates through
 * numpyro's MultivariateNormal.log_prob (gsmvi/monitors.py:107-113).  mu may be NULL (zero mean).  Monitor use
 * only (D dependent steps per row).  D <= 8192.
 */
int gsmvi_whiten_rows_f64(gsmvi_ctx* ctx, void* stream, int D, int nrows, const double* R, int ldr,
                          const double* X, int ldx, const double* mu, double* Z, int ldz, double* logdiag_dev);

/*
 * Draw samples X = 1 mu^T + Z R for whitened draws Z (B x D) and an upper factor R (R^T R = cov).
 * Replaces np.random.multivariate_normal(mean, cov, size=B) (gsm_numpy.py:116); Z is supplied by
 * the caller (host MT19937 stream in parity mode, device Philox in throughput mode).
 */
int gsmvi_sample_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                     const double* Z, int ldz, const double* mu, const double* R, int ldr,
                     double* X, int ldx);

/*
 * COLUMN-SHARDED factor-form GSM update (round 6; SURVEY 8(e) row 3 / (f) 3: the decomposition that divides the HBM-bound
 * D^2 passes and the D^2 memory of a fit by the number of ranks).  A rank owns the columns C = [col0, col0 + ncols) of the
 * square factor Fm (Sigma = Fm^T Fm) as a D x ncols block with its own leading dimension, and the entries C of the mean.
 *   gsmvi_sample_cols_f64          Xcols (B x ncols) = mu_cols + Z Fcols: the owned slice of x = mu + z Fm (gsm_numpy.py:116);
 *                                  the caller all-gathers the slices (B ncols doubles per rank).
 *   gsmvi_gsm_rows_stage_f64       on the block (D := ncols, nrows := D, G + col0, Fcols) gives the PARTIAL product
 *                                  G[:, C] Fm[:, C]^T (B x D); the caller all-reduces the partials to W = G Fm^T.
 *   gsmvi_gsm_factor_apply_cols_f64  from the replicated draws Z, the all-reduced W (B x D, contiguous) and the gathered
 *                                  samples X: the 2B x 2B chain of gsmvi_gsm_factor_update_f64 (replicated: identical inputs
 *                                  and arithmetic on every rank, so the accept / revert decision agrees) and the update of the
 *                                  OWNED block alone, Fcols' = Fcols + Rt^T (K'' Tm[:, C]), mu[C].  mu0 / mu are full-length
 *                                  vectors of which entries C are read / written.  col0 % 64 == 0, ncols % 64 == 0 (the last
 *                                  block may be ragged), even D and leading dimensions, 16-byte aligned blocks.
 * Per update a rank reads its block three times and writes it once (32 D ncols bytes) and exchanges B (ncols + D) doubles.
 */
int gsmvi_sample_cols_f64(gsmvi_ctx* ctx, void* stream, int D, int B, int ncols, const double* Z, int ldz,
                          const double* mu_cols, const double* Fcols, int ldf, double* Xcols, int ldx);
int gsmvi_gsm_factor_apply_cols_f64(gsmvi_ctx* ctx, void* stream, int D, int B, int col0, int ncols, const double* Z, int ldz,
                                    const double* W, const double* X, int ldx, const double* mu0, const double* F0cols,
                                    int ldf0, double* mu, double* Fcols, int ldf, int* info_dev, int* n_reverts_dev);

/*
 * COLUMN-SHARDED factor-form BaM update (bam.py:72-114 on a rank's columns C = [col0, col0 + ncols) of the square factor F0,
 * Sigma0 = F0^T F0; the same block layout and sampler as the GSM form above).  Per update:
 *   gsmvi_sample_cols_f64              the owned slice of x = mu0 + z F0, all-gathered by the caller (B ncols doubles per rank).
 *   gsmvi_bam_factor_wq_partial_f64    Wq_part (B x D, contiguous) = Qt[:, C] F0cols^T, Qt the B x D Helmert / gbar rows of G
 *                                      (sqrt(reg/B), sqrt(reg/(1+reg))); the caller all-reduces the partials to Wq = Qt F0^T
 *                                      (B D doubles).  wg = F0 gbar, which BaM's mean needs, is Wq's last row up to its scale.
 *   gsmvi_bam_factor_apply_cols_f64    from the replicated draws Z, the gathered samples X, the scores G and the all-reduced
 *                                      Wq: BaM's B x B chain and the 2B x 2B chain of gsmvi_bam_factor_update_f64 (replicated:
 *                                      identical inputs and arithmetic on every rank, so the accept / revert decision agrees),
 *                                      then Rt F0 on the block and the update of the OWNED block alone: Fcols = F0cols +
 *                                      Rt^T K'' (Rt F0cols), mu[C] = mu0[C]/(1+reg) + r1 (Sigma gbar)[C] + r1 xbar[C].
 *                                      mu0 / mu are full-length vectors of which entries C alone are read / written (mu0's
 *                                      other entries may be stale); on a revert *info_dev != 0, (mu[C], Fcols) = (mu0[C], F0cols)
 *                                      and *n_reverts_dev (may be NULL) is incremented.
 * With col0 = 0, ncols = D the two calls give gsmvi_bam_factor_update_f64's result.  col0 % 64 == 0, ncols % 64 == 0 (the
 * last block may be ragged), even D and leading dimensions, 16-byte aligned blocks, 2B <= min(D, 256); these are checked
 * (GSMVI_ERR_BAD_ARG / GSMVI_ERR_UNSUPPORTED) before the context is used.  No host synchronisation, graph-capturable, workspace
 * from the context (sized for (D, B)).  Per update a rank reads its block three times and writes it once and exchanges
 * B (ncols + D) doubles; the B x B and 2B x 2B chains and the B x D work are not divided.
 */
int gsmvi_bam_factor_wq_partial_f64(gsmvi_ctx* ctx, void* stream, int D, int B, int col0, int ncols, const double* G, int ldg,
                                    const double* F0cols, int ldf0, double reg, double* Wq_part);
int gsmvi_bam_factor_apply_cols_f64(gsmvi_ctx* ctx, void* stream, int D, int B, int col0, int ncols, const double* Z, int ldz,
                                    const double* X, int ldx, const double* G, int ldg, const double* Wq, const double* mu0,
                                    const double* F0cols, int ldf0, double reg, double* mu, double* Fcols, int ldf, int* info_dev,
                                    int* n_reverts_dev);

/*
 * Whitened draws: out[0..n) ~ N(0, 1), a pure function of (seed, call, element index) -- counter-based
 * Philox4x32-10 (key = seed, counter = (pair index, call)) + Box-Muller in fp64; see csrc/gsmvi_rng.hip.
 * Replaces the standard-normal stream behind np.random.multivariate_normal (gsm_numpy.py:105,116) in
 * throughput mode; `call` is the fit iteration (the JAX twins likewise derive a fresh sub-key per iteration,
 * gsm.py:117-119).  Stateless, so sharded ranks draw identical Z from the same key.  raw (device uint32,
 * 4 words per element pair, may be NULL) receives the Philox words (tests pin them to Random123 vectors).
 */
int gsmvi_randn_f64(gsmvi_ctx* ctx, void* stream, uint64_t seed, uint64_t call, int64_t n, double* out,
                    uint32_t* raw);

/*
 * The draws of SEVERAL consecutive calls from one launch: out[c * n + i] = element i of draw number call0 + c, c < ncalls --
 * bit-identical to ncalls calls of gsmvi_randn_f64 (a fit loop draws a block of iterations ahead: the stream does not depend
 * on the state).  call_in_dev (device uint64, may be NULL) is added to call0 on the device; call_out_dev (may be NULL, must
 * not alias call_in_dev) receives *call_in_dev + ncalls.  With the two words of a ping-pong pair a launch captured into a
 * hipGraph advances through the stream on every replay.
 */
int gsmvi_randn_batch_f64(gsmvi_ctx* ctx, void* stream, uint64_t seed, uint64_t call0, int ncalls, int64_t n, double* out,
                          const uint64_t* call_in_dev, uint64_t* call_out_dev);

/*
 * Commit-or-revert (gsm_numpy.py:121-125): if *info_dev == 0 copy (mu_new, S_new) over (mu, S),
 * else leave them; *n_reverts_dev is incremented on a revert.  Device-side, no host sync.
 */
int gsmvi_commit_f64(gsmvi_ctx* ctx, void* stream, int D, const int* info_dev,
                     const double* mu_new, const double* S_new, int lds_new,
                     double* mu, double* S, int lds, int* n_reverts_dev);

/*
 * BaM update (gsmvi/bam.py:72-114 with an exact rank-B factor of U; equals bam.py:31-69).
 * Symmetrised output (bam.py:199 does this in fit); jitter is added to the diagonal (bam.py:198).
 * The B x B matrix function of bam.py:108-110 (B + 1 columns in the reference's factorisation of U; an orthonormal
 * recombination of the centred score rows saves one without changing U) -- which the reference evaluates on the host through
 * jax.pure_callback (bam.py:15-22) -- runs on the device (scaled coupled Newton-Schulz square root on the MFMA pipe +
 * a one-workgroup Cholesky for B <= 129, the blocked Cholesky of gsmvi_potrf_f64 up to B = 1024 (round 6; 640 before); csrc/gsmvi_bam_small.hip):
 * no synchronisation, graph-capturable.  For B > 1024 the call returns GSMVI_ERR_UNSUPPORTED before anything is enqueued:
 * there is no host computation in this library.
 * *info_dev = 1 if that small problem was not finite / not positive definite (then mu, S are NaN-poisoned and the
 * caller's accept/revert must reject them).
 */
int gsmvi_bam_update_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                         const double* X, int ldx, const double* G, int ldg,
                         const double* mu0, const double* S0, int lds0, double reg, double jitter,
                         double* mu, double* S, int lds, int* info_dev);

/*
 * BaM update batch-sharded over RCCL (BASELINE config 4: B = 128 as 16 per GPU): BaM's statistics couple all samples, so the
 * ranks all-gather their (x_b, g_b) rows (two ncclAllGather of B_local x D doubles per rank) into xg_all (caller-owned,
 * 2 x B x D doubles: [X_all | G_all]) and every replica runs gsmvi_bam_update_f64 on the full batch; what is divided is the
 * score evaluation in front of it.  Validated before the first launch.
 */
int gsmvi_bam_update_sharded_f64(gsmvi_ctx* ctx, void* stream, void* nccl_comm, int D, int B_local,
                                 const double* X_local, int ldx, const double* G_local, int ldg,
                                 const double* mu0, const double* S0, int lds0, double reg, double jitter,
                                 double* xg_all, double* mu, double* S, int lds, int* info_dev);

/*
 * BaM update in FACTOR form (north_star's factor-form extension applied to gsmvi/bam.py:72-114): Sigma0 = F0^T F0 in,
 * Sigma = F^T F out, with F^T F equal to the S of gsmvi_bam_update_f64 (jitter = 0) to round-off and the same mean.  No D x D
 * covariance is formed and no D x D factorisation is taken: four passes over F0 and a 2B x 2B chain (the one of
 * gsmvi_gsm_factor_update_f64).  Z (B x D) are the whitened draws of the samples: X = mu0 + Z F0 (the caller's contract, as
 * for the GSM factor update).  Needs 2B <= min(D, 256) (GSMVI_ERR_UNSUPPORTED otherwise, before anything is enqueued).
 * *info_dev != 0 and (mu, F) = (mu0, F0) if BaM's B x B matrix function or the 2B x 2B chain failed (non-finite input, or a
 * Sigma that is not positive definite to working precision); *n_reverts_dev (may be NULL) is then incremented.  Since round 5
 * the update works in the basis [Vw; Zt] (Zt: the part of Zw orthogonal to the whitened draws), which takes the Cholesky factor
 * of Gvv = Vw Vw^T: LINEARLY DEPENDENT draws (a repeated sample; impossible for i.i.d. normal draws, legal in bam.py) make Gvv
 * singular -- the update then either still equals the dense one or is reverted with *info_dev != 0; ALMOST dependent draws
 * ((max R_ii / min R_ii)^2 > 1e8 on the factor's diagonal) are reverted too, because the basis is orthogonal only to
 * eps cond(Gvv).  That ratio is a HEURISTIC LOWER BOUND of cond(Gvv), not the condition number (a graded matrix of Kahan's
 * kind has a far larger one): it catches what it was built for -- one draw nearly repeating another, 5e-6 off without a flag at
 * cond 1e12 before the guard (tests/test_gpu_bam.py) -- and is no guarantee for adversarial draws; method="dense" has no
 * such precondition.
 */
int gsmvi_bam_factor_update_f64(gsmvi_ctx* ctx, void* stream, int D, int B,
                                const double* Z, int ldz, const double* X, int ldx, const double* G, int ldg,
                                const double* mu0, const double* F0, int ldf0, double reg,
                                double* mu, double* F, int ldf, int* info_dev, int* n_reverts_dev);

/*
 * Factor-form BaM update batch-sharded over RCCL (BASELINE config 4, "B = 128 sharded 16/GPU", without a D x D covariance or a
 * D^3 step on any rank; round 4).  Z_all (B x D, B = B_local x ranks) are the whitened draws of ALL samples, replicated (every
 * rank draws the same counter-based stream, gsmvi_randn_f64); X_local / G_local are the samples and scores of this rank's
 * rows [rank B_local, (rank + 1) B_local).  As in gsmvi_bam_update_sharded_f64 the (x_b, g_b) rows are all-gathered into
 * xg_all (caller-owned, 2 x B x D doubles) and every replica runs gsmvi_bam_factor_update_f64 on the full batch: replicas stay
 * bit-identical.  Geometry and the 2B <= min(D, 256) bound are validated before the first launch.
 */
int gsmvi_bam_factor_update_sharded_f64(gsmvi_ctx* ctx, void* stream, void* nccl_comm, int D, int B_local,
                                        const double* Z_all, int ldz, const double* X_local, int ldx,
                                        const double* G_local, int ldg, const double* mu0, const double* F0, int ldf0,
                                        double reg, double* xg_all, double* mu, double* F, int ldf, int* info_dev,
                                        int* n_reverts_dev);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* GSMVI_HIP_H */
