/*
 * ggl_hip.h -- C ABI of libggl_hip.so: the MI355X (gfx950) ADMM inner loop for General Graphical
 * Lasso.  This is the drop-in boundary for the hot path of fabian-sp/GGLasso; every entry point
 * names the reference interface it replaces (paths relative to /root/reference/src/gglasso/).
 *
 * Conventions
 *   - All matrices are float64, C-contiguous, row-major; stacks are (K,p,p) with k slowest.
 *   - "host" pointers are ordinary CPU memory owned by the caller (NumPy arrays); the library
 *     owns every device buffer inside the opaque ggl_ctx and never keeps a host pointer.
 *   - Every function returns 0 on success, <0 on error (GGL_E_*); ggl_last_error() returns a
 *     thread-local message.  No C++ exception crosses the ABI.
 *   - A ctx is bound to one device and one HIP stream and is not thread-safe.  Multi-GPU = one
 *     process (rank) per GPU, each with its own ctx (see gglasso_amd/dist.py).
 *   - Eigenvector matrices cross the ABI in NumPy's convention: Q (K,p,p) with eigenvectors in
 *     COLUMNS, eigenvalues ascending (numpy.linalg.eigh, called at solver/admm_solver.py:181,199).
 */
#ifndef GGL_HIP_H
#define GGL_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version: major * 100 + minor.  Bumped whenever an entry point changes its argument layout or an existing buffer its
 * format -- 300 (round 6): ggl_pipeline_stats writes out[10] (was out[5]), GGL_BUF_GROUPSQ is the packed upper triangle with
 * the flag at p (p + 1) / 2 (was (p,p) + 1), the int8 entry points live in the development library only, ggl_debug_poison
 * takes a byte pattern.  A binding built against another major version must refuse to load (gglasso_amd/_lib.py does).
 * Entry points and selector values that are only ADDED (GGL_REG_FSGL, ggl_set_block_size, ggl_prox_sum_frob,
 * ggl_frob_norm_per_block, ggl_fsgl_stats, ggl_covariance, ggl_scale_by_diagonal, ggl_set_S_from_data, ggl_get_S, ggl_kkt_terms,
 * ggl_diag_stats, ggl_covariance_subsets, ggl_set_S_from_subsets, ggl_edge_stability, ggl_kendall_counts, ggl_kendall_skeptic,
 * ggl_set_S_from_kendall, ggl_covariance_pairwise, ggl_covariance_pairwise_subsets, ggl_set_S_from_data_pairwise,
 * ggl_set_S_from_subsets_pairwise, ggl_covariance_weighted, ggl_set_S_from_weighted, ggl_mixed_correlation,
 * ggl_set_S_from_mixed, ggl_nearest_correlation, ggl_project_S, ggl_heldout_scores, ggl_debias, ggl_cholesky_predict,
 * ggl_weighted_predictive_scores, ggl_neighborhood_path, ggl_neighborhood_stability, ggl_neighborhood_refit,
 * ggl_neighborhood_cv, ggl_mb_refit_limits, ggl_neighborhood_path_w, ggl_neighborhood_stability_w, ggl_neighborhood_cv_w, ggl_neighborhood_joint_path,
 * ggl_neighborhood_joint_last, ggl_mb_joint_limits, ggl_mb_joint_chunk_budget, ggl_dev_mb_joint_bench,
 * ggl_neighborhood_fused_path, ggl_neighborhood_fused_last, ggl_mb_fused_limits, ggl_dev_mb_fused_bench) leave every existing layout alone and the number where it is. */
#define GGL_VERSION 300

/* error codes */
#define GGL_OK 0
#define GGL_E_ARG (-1)      /* bad argument (the reference would raise AssertionError) */
#define GGL_E_HIP (-2)      /* HIP runtime error */
#define GGL_E_SOLVER (-3)   /* rocSOLVER / eigensolver did not converge */
#define GGL_E_ALLOC (-4)
#define GGL_E_COMM (-5)     /* RCCL error, or librccl could not be loaded */

/* penalty selector: reg argument of ADMM_MGL (solver/admm_solver.py:13-31) / ADMM_SGL */
#define GGL_REG_SGL 0       /* K independent single problems: prox_od_1norm (ggl_helper.py:16-27) */
#define GGL_REG_GGL 1       /* prox_phi_ggl (ggl_helper.py:68-71) */
#define GGL_REG_FGL 2       /* prox_phi_fgl (ggl_helper.py:131-134) */
#define GGL_REG_FSGL 3      /* K independent Functional SGL problems, ADMM_FSGL (solver/functional_sgl_admm.py:12-238): prox_sum_Frob
                             * (ggl_helper.py:45-66) over the M x M blocks of ggl_set_block_size */

/* eigensolver selector (ctx flags, low byte) */
#define GGL_EIG_AUTO 0      /* p <= GGL_NS_MIN_P: LDS Jacobi for everything.  Larger p: Newton-Schulz matrix functions for the
                             * Omega-step and the L-step; where eigenvalues themselves are needed (exit checks, KKT, objective,
                             * selection statistics, the final L, fallbacks) LDS Jacobi up to GGL_JACOBI_MAX_P, rocSOLVER above. */
#define GGL_EIG_JACOBI 1    /* hand-written one-workgroup-per-matrix Jacobi (p <= GGL_JACOBI_MAX_P) */
#define GGL_EIG_ROCSOLVER 2 /* rocsolver_dsyevd_strided_batched */
#define GGL_EIG_NEWTON_SCHULZ 3 /* Omega-step without an eigendecomposition: Omega = (W + sqrt(W^2+4 beta I))/2
                                 * by scaled Newton-Schulz products on the FP64 matrix cores (any p).
                                 * Steps that need eigenvalues themselves (L-step, exit checks) use AUTO. */
#define GGL_JACOBI_MAX_P 128
#define GGL_NS_MIN_P 8        /* GGL_EIG_AUTO: Omega- / L-step by Newton-Schulz matrix functions for p > this (measured crossover) */
/* Newton-Schulz controls in the bits above the selector (ctx flags and the eig_method argument of the stateless
 * ggl_phiplus_matrix / ggl_rank_matrix): product mode 0 auto (by condition number), 1 all-symmetric products,
 * 2 stable unsymmetrised products; highest step degree 3, 5 or 9 (0 = 9).  Used by the parity tests to reach every
 * schedule; the solvers pass neither. */
#define GGL_EIG_NS_MODE(m) (((m) & 0x3) << 8)
#define GGL_EIG_NS_DEGREES(d) (((d) & 0xf) << 12)
/* ctx flag: the `stream` argument of ggl_ctx_create is the caller's stream even when the handle is NULL (the legacy
 * default stream -- what torch.cuda.current_stream().cuda_stream is for torch's default stream).  Without the bit a
 * NULL handle means "create a private non-blocking stream", which has NO implicit ordering with the NULL stream. */
#define GGL_CTX_STREAM_GIVEN (1 << 16)

/* which-buffer selector of ggl_device_ptr */
#define GGL_BUF_S 0
#define GGL_BUF_OMEGA 1
#define GGL_BUF_THETA 2
#define GGL_BUF_L 3
#define GGL_BUF_X 4
#define GGL_BUF_GROUPSQ 5   /* partial sum_k u^2 of the GGL Theta-step (K-sharded runs): PACKED upper triangle, row-major with the
                             * diagonal, element (i,j), i <= j, at i p - i (i - 1) / 2 + (j - i): p (p + 1) / 2 doubles, + 1 flag double */
#define GGL_BUF_NORMS 6     /* (K,5) per-instance squared norms of the stopping test */
#define GGL_BUF_OMEGA_PREV 7

typedef struct ggl_ctx ggl_ctx;

int ggl_version(void);
const char *ggl_last_error(void);
/* number of visible HIP devices, or <0 (used by the loader to fail loudly on a GPU-less box) */
int ggl_device_count(void);

/* ---- context ---------------------------------------------------------------------------------
 * Replaces the NumPy temporaries ADMM_MGL allocates per call (admm_solver.py:142-154).
 * stream: an existing hipStream_t or NULL to create one (see GGL_CTX_STREAM_GIVEN for the NULL stream itself). */
int ggl_ctx_create(int device, int K, int p, int flags, void *stream, ggl_ctx **out);
int ggl_ctx_destroy(ggl_ctx *ctx);          /* (NULL: a no-op that succeeds, like free) */
int ggl_ctx_sync(ggl_ctx *ctx);
void *ggl_device_ptr(ggl_ctx *ctx, int which);

/* ctx options.  The shipped library reads NO environment variables: every dispatch decision is a function of the
 * problem shape and of these options (defaults in brackets).  None of them changes what is computed, only how; the
 * parity tests run the iteration under each setting.  (A GGL_DEV build of the library -- libggl_hip_dev.so, used by
 * tools/ -- additionally maps the environment variables GGL_SPECULATE, GGL_SPEC_FACTOR, GGL_NS_MODE, GGL_NS_DEGREES,
 * GGL_THETA_FLAT, GGL_RANK_EIG, GGL_TWO_STREAM, GGL_PARTS_MAX_TILES, GGL_SYMM_VARIANT, GGL_SPIN_WAIT,
 * GGL_FUSED_BOUNDS, GGL_PIPELINE, GGL_FUSED_START, GGL_PARTS_SMALL onto them.) */
/* Options marked DEV are the measured-and-rejected alternatives of rounds 2-5 (each built, bit-identical or parity-tested, and
 * slower or within noise: DESIGN.md 8.1, 9.7, 9.10, 10.7).  Since round 6 they exist in the development library only
 * (libggl_hip_dev.so); the product library accepts the value 0 for them and refuses anything else with GGL_E_ARG. */
#define GGL_OPT_SPECULATE 1        /* [1] speculative Omega-step (schedule from the previous iteration's bounds)     */
#define GGL_OPT_SPEC_FACTOR 2      /* [1.02] inflation of the previous bounds; < 1 forces validation misses (tests)  */
#define GGL_OPT_NS_MODE 3          /* [0] as GGL_EIG_NS_MODE                                                          */
#define GGL_OPT_NS_DEGREES 4       /* [9] as GGL_EIG_NS_DEGREES                                                       */
#define GGL_OPT_THETA_FLAT 5       /* [2] GGL Theta-step for exactly symmetric states, K <= 32: 0 tile-pair kernels, 1 per-element
                                    * kernel, 2 per-element kernel with the K-column split over the four waves of a workgroup */
#define GGL_OPT_RANK_EIG 6         /* [0] L-step by eigendecomposition instead of the sign iteration                 */
#define GGL_OPT_PARTS 7            /* [2] parts of the batch that run their launch sequences concurrently (1..4)     */
#define GGL_OPT_PARTS_MAX_TILES 8  /* [2048] concurrent parts only up to this many 64x64 tile pairs in the batch     */
#define GGL_OPT_SYMM_VARIANT 9     /* [-1 = by size] product-kernel instance, see csrc/gemm_sym.hip                   */
#define GGL_OPT_SPIN_WAIT 10       /* [1] wait for the end of an iteration by polling a pinned sequence number       */
#define GGL_OPT_FUSED_BOUNDS 11    /* [1] spectral-bound partials from the epilogue of the product launch (no norm pass) */
#define GGL_OPT_PIPELINE 12        /* [1] ggl_admm_step launches the next iteration's Omega-step chain before it returns     */
#define GGL_OPT_FUSED_START 13     /* [1] speculative step: the first step's start matrix is the B' launch's second output   */
#define GGL_OPT_PARTS_SMALL 14     /* [8] smallest batch below 16 (p >= 384) that still runs as two concurrent parts; 0 = none */
#define GGL_OPT_NS_TOL 15          /* [2e-12] relative spectral accuracy the Omega-step's matrix square root is iterated to:
                                    * |Omega - phiplus(W)|_2 <= tol * |sqrt(W^2 + 4 beta I)|_2 / 2 (+ rounding).  0 (or anything
                                    * below 4e-16) iterates to fp64 resolution: results then agree with eigh to ~1e-13 at one
                                    * more product per iteration around condition number 2.  Measured at GGL (32,500), solved
                                    * to 1e-10: |Theta - reference|_F = 1.3e-10 (default) / 2.8e-13 (exact) on a stack of norm
                                    * 128; the reference comparison asks for 1e-8.  The stateless ggl_phiplus_matrix is exact. */
#define GGL_OPT_CW_WARM 16         /* [1] the Collatz-Wielandt weight vector of the spectral bound is carried from one iteration to
                                    * the next (a power iteration at no extra pass; the bound stays rigorous and tightens
                                    * towards the Perron root of |B'|); 0: the row sums of |B'| every time                  */
#define GGL_OPT_CHAIN 17           /* RETIRED [0]: the persistent chain was removed; both libraries take 0, refuse
                                    * anything else and report 0.  What it was -- 1: speculative Omega-steps of batches that cover the XCDs (K >= 8, even p, >= 1100 64x64 tile
                                    * pairs) run their whole product chain as ONE persistent launch with per-instance
                                    * dependencies (k_omega_chain, csrc/gemm_sym.hip) instead of one launch per product in
                                    * concurrent parts; 2: wherever it can run (any K >= 8, even p).  Same products, same bits
                                    * (tests/test_gpu_chain.py, removed with it).  Measured SLOWER on MI355X (headline Omega
                                    * phase 0.89 vs 0.72 ms; DESIGN.md section 8.1, profiles/r3_omega_chain_*.txt)           */
#define GGL_OPT_RANK_DEFLATE 20    /* [1] L-step (sign iteration): after a first pass at GGL_OPT_RANK_L0_DEFLATE the eigenvalues next to the
                                      threshold are deflated (range of I - X^2, exact small problem) instead of iterated down */
#define GGL_OPT_RANK_L0_DEFLATE 21 /* [2e-3] resolution of that first pass */
#define GGL_OPT_FUSED_CW 22        /* DEV [0] the bound validation of a speculative Omega-step (row sums + Collatz-Wielandt pass) as ONE launch:
                                      built in round 4 for the small slabs, measured equal there and slower at the headline */
#define GGL_OPT_OMEGA_LDS 23       /* [1] p <= 64: the whole Omega-step as ONE launch, one workgroup per instance, the Newton-Schulz chain
                                      resident in LDS, bound and per-instance schedule chosen on the device (omega_lds.hip); an instance
                                      outside its range (condition number of W^2 + 4 beta I above 300) sends the step to the launch chain.
                                      1: waves per workgroup by size (8, i.e. two per SIMD, for 32 < p <= 64; round 5), 4 / 8: that many */
#define GGL_OPT_EARLY_PART 24      /* [1] with GGL_OPT_PIPELINE, ggl_admm_step: the first part of the NEXT iteration's Omega-step chain (tables,
                                      W, A', B': scratch only) goes into the stream before the host waits for this iteration's residuals,
                                      on the prediction that the rho rule keeps rho; its schedule is built from the bounds validated one
                                      iteration earlier, so iterates agree with GGL_OPT_EARLY_PART = 0 to the Omega-step's tolerance */
#define GGL_OPT_FUSED_W 26         /* [1] with GGL_OPT_EARLY_PART, GGL, exactly symmetric state and S: the Theta kernel that precedes an early
                                      first part also writes that part's W = Theta - X - beta S (admm_solver.py:180) from the values it
                                      holds -- one pass over three stacks and one launch per part less (round 5) */
#define GGL_OPT_RANK_CW 27         /* DEV [0] L-step (sign iteration): the norm bound |C|_2 from a Collatz-Wielandt pass over C C with a vector
                                      carried across ADMM iterations (as the Omega-step's bound) instead of sqrt(min(|C C|_inf, |C C|_F)).
                                      Built and measured in round 5 (FGL K=50, p=500, latent): the schedule is a step function of the
                                      resolution -- 22.0 products with either bound at GGL_OPT_RANK_L0_DEFLATE = 2e-3, 21.4 / 20.8 at
                                      4e-3 where 3-4x as many instances need the continuation -- and the pass costs 25 us: 211 it/s
                                      without, 202 with.  Off. */
#define GGL_OPT_BOUND_SIDE 28      /* DEV [0] speculative Omega-step: the two kernels that validate the assumed bound run on a side stream beside the
                                      chain's first products, joined before B' is overwritten (round 5).  0 off, 1 on, 2 only for two
                                      concurrent parts of a large batch.  Bitwise the in-chain order; measured: the small launch-bound
                                      sequences lose 2-5 % to the cross-stream waits, the headline gains 0.8 % over nine A/B pairs
                                      whose scatter is +-2 % (profiles/r5_bound_side.txt): off */
#define GGL_OPT_LDS_PINNED 29      /* [1] p <= 64: the LDS-resident kernels (and the Theta kernel of a batched grid behind them) read their per-step
                                      parameters from the pinned host mirror instead of waiting for a copy kernel in front of them */
#define GGL_OPT_JOIN_FLAG 30       /* [1] concurrent parts of a speculative Omega-step are joined through flag words in device memory (a one-wave
                                      kernel on the main stream polls what the parts' streams set behind their last launch) instead of a
                                      cross-queue event wait, which idles the waiting queue ~25 us after the event has fired */
#define GGL_OPT_CW_RIDER 31        /* [1] speculative Omega-step: the validation of the assumed spectral bound (row sums, Collatz-Wielandt ratio,
                                      Frobenius norm of B' = A'^2) runs as extra workgroups of the first product launch after B' instead of two
                                      dependent launches in front of it (the schedule does not wait for it; small launch sequences leave most
                                      CUs idle).  Same arithmetic, same bound.  2: the rider as a launch of its own (what a chain without such a
                                      product launch gets; for tests). */
#define GGL_OPT_COPY_RIDER 32      /* [1] the small host-to-device table transfers in front of an Omega-step chain (schedule coefficients, assumed bounds,
                                      flag zeroing) ride in the A' = W^2 + 4 beta I launch as extra workgroups when nothing else is pending and the
                                      device's coefficient rows of A' are already those of this beta: one dependent launch less per iteration.  1 = where the
                                      chain is ONE launch sequence (two concurrent parts measured slower with it), 2 = always, 0 = never */
#define GGL_OPT_REDUCE_RIDER 33    /* [2] the norm reduction behind a Theta-step rides in the A' launch of the next chain's early first part (one extra
                                      workgroup; same sums in the same order) when that launch follows it in the stream anyway: one dependent
                                      launch less per iteration.  1 = single launch sequences, 2 = always, 0 = never */
#define GGL_OPT_PARTS_BIAS 34      /* DEV [0] two concurrent parts of an Omega-step take K/2 + bias and K/2 - bias instances (the second part starts and
                                      ends ~40 us after the first) */
#define GGL_OPT_PARTS_ORDER 35     /* DEV [0] two concurrent parts: 1 = the part on the ctx's main stream is queued after the other one */
#define GGL_OPT_DOWNLOAD_THREADS 36 /* [8] ggl_get_state / ggl_get_snapshots of more than 32 MB: host threads that touch the pages of the caller's
                                      (typically freshly allocated) arrays before the copy -- the first touch, not the transfer, is what a
                                      download into new memory waits for; 1 = none */
#define GGL_OPT_GROUP_SCHED 37     /* [1] a batch whose instances need different product counts for their matrix square root (a grid of
                                      independent problems: the reference solves every point with its own eigh, helper/model_selection.py:
                                      619-633) runs as up to 3 contiguous groups with their own Newton-Schulz schedules -- the concurrent
                                      parts of the engine -- where the size rule would run it as one launch sequence on the worst
                                      instance's schedule; taken when a deterministic time model gains >= 6 %.  0 off, 2 / 3 = at most
                                      that many groups; 12 / 13 (tests) = at most 2 / 3 groups wherever the product counts differ */
#define GGL_OPT_OMEGA_POLY 38      /* [1] a launch sequence of the Omega-step (part or group) whose spectral interval and ns_tol let ONE
                                      polynomial in A' (degree 6 / 9 / 12 / 15, Paterson-Stockmeyer evaluation: 4 / 5 / 6 / 7 products,
                                      A' and B' included) meet the tolerance with strictly fewer products than the Newton-Schulz
                                      schedule runs that polynomial instead; 0 = Newton-Schulz everywhere */
#define GGL_OPT_PART_PRIORITY 25   /* DEV [0] streams of the concurrent parts of an Omega-step: 0 = created like any stream, 1 = with the highest,
                                      2 = with the lowest stream priority (streams of another priority never share a hardware queue with
                                      the ctx's main stream) */
#define GGL_OPT_ISOLATE 19         /* [0] batches of independent problems: an instance whose data turn non-finite or whose eigensolver
                                      does not converge is marked (ggl_failed_instances) instead of failing the call */
#define GGL_OPT_RANK_L0_COARSE 18  /* [8e-5] two-tier L-step (sign iteration, p > GGL_JACOBI_MAX_P): the first pass over the whole batch
                                    * resolves eigenvalues of C down to this distance from the threshold (relative to |C - mu I|);
                                    * the instances whose residual check says that was not enough are continued, from the iterate
                                    * they have, as a compact sub-batch down to the resolution of the one-tier run (1e-6).  The
                                    * schedule's length is set by the WORST instance of a batch and its degree sequence is common
                                    * to a launch: at K = 50, p = 500 the batch needs 1e-6, nine instances in ten 1e-4
                                    * (28 instead of 37 products).  Measured there (with the norm bound from C^2): 154 -> 175 it/s,
                                    * flat for 5e-5 .. 1e-4.
                                    * 0: one tier.                                                                            */
int ggl_ctx_set_option(ggl_ctx *ctx, int option, double value);
int ggl_ctx_get_option(ggl_ctx *ctx, int option, double *value);

/* ---- state upload / download ----------------------------------------------------------------
 * S: admm_solver.py:13 (argument S).  set_state: Omega_0/Theta_0/X_0 copies, admm_solver.py:142-150
 * (NULL leaves the buffer as is; L NULL zeroes it like admm_solver.py:149).  get_state: the `sol`
 * dict of admm_solver.py:303 (NULL = skip). */
int ggl_set_S(ggl_ctx *ctx, const double *S_host);
int ggl_set_state(ggl_ctx *ctx, const double *Omega, const double *Theta, const double *L,
                  const double *X);
/* The same with arrays SHARED by the instances of a batch: `period` / periods[0..3] (Omega, Theta, L, X; NULL = all 0) is the
 * number of instances the host array holds -- 0: all K; P > 0 (a divisor of K, anything else is GGL_E_ARG): P, and instance k of the
 * ctx is its instance k % P.  P = 1: one (p,p) matrix for all (the grid of single_grid_search starts every instance from the same S, Omega_0, X_0);
 * P = K': the stack of ONE multiple-graph problem for each of the G grid points of grid_search.  Uploaded once, replicated on
 * the device. */
int ggl_set_S_ex(ggl_ctx *ctx, const double *S_host, int period);
int ggl_set_state_ex(ggl_ctx *ctx, const double *Omega, const double *Theta, const double *L, const double *X,
                     const int *periods);
int ggl_get_state(ggl_ctx *ctx, double *Omega, double *Theta, double *L, double *X);
/* restore == 0: keep a device copy of the iterate; != 0: make it the iterate again (ggl_set_state with the arrays of that
 * moment, without the host round trip; everything carried from earlier iterations is forgotten, as in ggl_set_state). */
int ggl_state_snapshot(ggl_ctx *ctx, int restore);
/* lambda1 * lambda1_mask as a (p,p) array (single_admm_solver.py:114); NULL clears it. */
int ggl_set_lambda1_mask(ggl_ctx *ctx, const double *lam_pp_host);

/* ---- one ADMM iteration ---------------------------------------------------------------------
 * Body of the hot loop, admm_solver.py:179-224 / single_admm_solver.py:163-193:
 *   W = Theta - L - X - (nk/rho) S ; (D,Q) = eigh(W) ; Omega = phiplus(nk/rho, D, Q)
 *   Theta = prox_p(Omega + L + X, lambda1/rho, lambda2/rho, reg)      (prox_od_1norm for SGL)
 *   latent: L = prox_rank_norm(Theta - X - Omega, mu1/rho)
 *   X += Omega - Theta + L
 * out_norms[5] = squared Frobenius norms over the whole stack that ADMM_stopping_criterion
 * (admm_solver.py:316-331) needs: |Omega|^2, |Theta-L|^2, |X|^2, |Omega-Theta+L|^2,
 * |Omega-Omega_prev|^2.  rho update and the stopping decision stay on the host (admm_solver.py:227-246).
 * mu1: host (K,) or NULL; nk: host (K,) or NULL (= ones).  rho, lambda1 are per-iteration scalars.
 * For p > 128 the Omega- and L-steps are matrix-function iterations on the FP64 matrix cores; with
 * the same rho as in the previous call the Omega-step runs on a schedule built from that call's spectral bounds
 * and is validated on the device -- a rejected step leaves the iterate untouched and is repeated inside this call
 * (GGL_OPT_SPECULATE 0 switches that off).  One host synchronisation per call in the common case.  With GGL_OPT_PIPELINE
 * the call also launches the NEXT iteration's Omega-step chain for the same rho before it returns whenever the
 * reference's rho rule (admm_solver.py:227-233) would keep rho for the residuals just computed; the next call takes the
 * chain over if its rho (and nk) are the same and drops it otherwise, and every other entry point drops it first. */
int ggl_admm_step(ggl_ctx *ctx, double rho, double lambda1, double lambda2, int reg, int latent,
                  const double *mu1, const double *nk, double out_norms[5]);
/* The caller's loop ends after the next ggl_admm_step (max_iter reached, admm_solver.py:172): that call does not
 * pre-launch a chain nobody would take over.  One-shot; without it the unused chain is merely dropped by the next
 * entry point. */
int ggl_hint_last_step(ggl_ctx *ctx);

/* The same iteration split at the one point where a K-sharded GGL run has to exchange data
 * (sum_k u^2 couples the shards, ggl_helper.py:38-43):
 *   ggl_step_omega          Omega-step on the local K-slab
 *   ggl_step_group_partial  u = soft(Omega+L+X, l1/rho); GROUPSQ = packed upper triangle of sum_{local k} u^2  (GGL only)
 *   -- caller all-reduces GGL_BUF_GROUPSQ over ranks (RCCL) --
 *   ggl_step_finish         Theta from the reduced GROUPSQ, L-step, X update, local norms       */
int ggl_step_omega(ggl_ctx *ctx, double rho, int latent, const double *nk);
int ggl_step_group_partial(ggl_ctx *ctx, double rho, double lambda1);
/* ggl_step_omega that may run speculatively (schedule from the previous iteration's bounds, no host sync).  The
 * validation flag of this rank is appended to GROUPSQ as element p(p+1)/2 by ggl_step_group_partial, so the caller's
 * all-reduce must cover p(p+1)/2 + 1 doubles; ggl_step_finish reads the reduced flag back and, if ANY rank missed, leaves
 * the iterate alone; ggl_norms_read (or ggl_step_finish without deferred norms) then returns 1 on every rank:
 * repeat the iteration with ggl_step_omega. */
int ggl_step_omega_spec(ggl_ctx *ctx, double rho, int latent, const double *nk);
int ggl_step_finish(ggl_ctx *ctx, double rho, double lambda1, double lambda2, int reg, int latent,
                    const double *mu1, int groupsq_ready, double out_norms[5]);
/* groupsq_ready bit 1 (value 2): leave the five local sums in the NORMS buffer instead of returning them, so that
 * a K-sharded run can all-reduce them on the device (no host round trip); ggl_norms_read then copies them out
 * (one stream sync), exactly what ggl_step_finish does itself without the bit. */
int ggl_norms_read(ggl_ctx *ctx, double out_norms[5]);

/* ---- RCCL behind the ABI: the K-sharded GGL iteration as one call -------------------------------
 * One process per GPU, each with a ctx over its K-slab.  librccl.so.1 is resolved at run time
 * (dlopen), libggl_hip.so does not link it.
 *   ggl_comm_unique_id  ncclGetUniqueId on one rank; the host program distributes the 128 bytes by its own means
 *                       (MPI_Bcast, a file, torch.distributed's store -- gglasso_amd/dist.py uses broadcast_object_list)
 *   ggl_comm_init       ncclCommInitRank for this ctx's device; the collectives run on the ctx stream
 *   ggl_admm_step_sharded  the whole iteration of admm_solver.py:179-224 on this rank's slab with its two exchanges:
 *                       Omega-step (speculative) | local sum_k u^2 -> ncclAllReduce of GROUPSQ (p(p+1)/2 + 1 doubles: the
 *                       packed upper triangle, the validation flag rides along) | Theta-step, dual update, five local sums -> ncclAllReduce (5
 *                       doubles) | one host synchronisation.  out_norms are the GLOBAL sums: every rank takes the same
 *                       rho / stopping decision.  A rejected speculative step is repeated inside the call on all ranks.
 *   ggl_allreduce_groupsq / ggl_allreduce_norms  the two collectives alone, for callers that use the split entry points. */
int ggl_comm_unique_id(char id_out[128]);
int ggl_comm_init(ggl_ctx *ctx, int rank, int nranks, const char id[128]);
int ggl_comm_destroy(ggl_ctx *ctx);
/* ncclCommCount of the ctx's communicator: the number of ranks RCCL itself sees (bench.py reports it as n_ranks_seen) */
int ggl_comm_count(ggl_ctx *ctx, int *nranks_out);
int ggl_allreduce_groupsq(ggl_ctx *ctx);
int ggl_allreduce_norms(ggl_ctx *ctx);
int ggl_admm_step_sharded(ggl_ctx *ctx, double rho, double lambda1, double lambda2, const double *nk,
                          double out_norms[5]);
/* the same with latent variables (admm_solver.py:197-208): the L-step and the dual update are per instance, so they run on
 * the local slab between the Theta-step (reduced group sums) and the all-reduce of the five sums; mu1 (K_local,).  A latent
 * step neither speculates nor pre-launches (the L-step has its own verification synchronisation). */
int ggl_admm_step_sharded_latent(ggl_ctx *ctx, double rho, double lambda1, double lambda2, int latent,
                                 const double *mu1, const double *nk, double out_norms[5]);

/* ---- K independent single problems (batched lambda path) ---------------------------------------
 * The ctx stack is used as K separate ADMM_SGL problems (single_admm_solver.py:157-214), each with its
 * own rho_k and lambda1_k -- what the outer loop of single_grid_search (helper/model_selection.py:619-630)
 * solves one after the other.  out_norms is (K,5): the five squared norms per instance.
 * ggl_scale_X_batch: X_k <- factor_k X_k.  ggl_get_state_k: one instance of the state (snapshot at the
 * iteration it converged). */
int ggl_sgl_batch_step(ggl_ctx *ctx, const double *rho, const double *lambda1, int latent,
                       const double *mu1, double *out_norms);
/* The batch as problems of DIFFERENT dimension -- the connected components block_SGL solves one after the other
 * (single_admm_solver.py:422-459): instance k is the leading (pk[k],pk[k]) block of its (p,p) slot, the caller pads the rest of
 * S, Omega, Theta with an identity block and X with zeros (a decoupled fixed point of the iteration, as for ggl_ext_*);
 * ggl_sgl_batch_step's five sums then run over the block only, so every instance stops exactly where its own ADMM_SGL
 * would.  NULL: all instances have dimension p again.  Not with latent variables.
 * ggl_set_lambda1_mask_k: one (p,p) threshold array lambda1 * lambda1_mask PER INSTANCE, (K,p,p) (block_SGL hands every
 * component its own slice of the mask, :447); NULL clears it (the shared mask of ggl_set_lambda1_mask applies again). */
int ggl_set_instance_dims(ggl_ctx *ctx, const int *pk);
/* Functional SGL (solver/functional_sgl_admm.py:12-238; argument M, :14): every (p,p) instance of the ctx is a (p/M) x (p/M)
 * grid of M x M blocks and the Theta-step is prox_sum_Frob (solver/ggl_helper.py:45-66, called at functional_sgl_admm.py:147):
 * off-diagonal blocks shrunk by their Frobenius norm (prox_2norm, ggl_helper.py:38-43; the upper block decides, the lower
 * one is its transpose), diagonal blocks passed through.  M has to divide p (:102, GGL_E_ARG otherwise); M = 0 clears it.
 *   ggl_admm_step / ggl_step_finish / ggl_objective with GGL_REG_FSGL: one problem per instance with the same lambda1;
 *     the penalty of ggl_objective is lambda1 sum_{I != J} |Theta_IJ|_F (:36).  GGL_E_ARG without a block size.
 *   ggl_sgl_batch_step / ggl_sgl_batch_run with a block size set: the block penalty instead of the element-wise one, one
 *     lambda1 per instance -- a lambda path of ADMM_FSGL problems as one batch.  The fused one-launch iteration of p <= 64
 *     (element-wise shrink) is not requested then; the LDS-resident Omega-step alone still runs.
 *   GGL_E_ARG, before anything is launched: a block size together with ggl_set_lambda1_mask / ggl_set_lambda1_mask_k, or with
 *     ggl_set_instance_dims.  The reference's ADMM_FSGL has no KKT stopping criterion: ggl_kkt_residual refuses GGL_REG_FSGL.
 * M <= 32: one launch over tile pairs of edge M floor(32/M); M > 32: a table of block sums first, then the same kernel
 * (csrc/theta_fsgl.hip).  Deterministic: fixed reduction order, no floating-point atomics. */
int ggl_set_block_size(ggl_ctx *ctx, int M);
int ggl_set_lambda1_mask_k(ggl_ctx *ctx, const double *lam_Kpp_host);
int ggl_scale_X_batch(ggl_ctx *ctx, const double *factor);
int ggl_get_state_k(ggl_ctx *ctx, int k, double *Omega, double *Theta, double *L, double *X);

/* ---- G independent multiple-graph problems on the same S (batched lambda1 x lambda2 grid) -----------
 * What the MAIN LOOP of grid_search (helper/model_selection.py:208-224) solves one (lambda1, lambda2) point after the
 * other: here the ctx stack holds G problems of K/G instances each, problem g in the slots g*K/G .., every problem with
 * its own rho_g, lambda1_g, lambda2_g; one call = one ADMM_MGL iteration (admm_solver.py:179-224) of all of them
 * (batched Omega-/L-step over all G*K/G matrices, one Theta-step launch with a grid-point dimension).  mu1: (K total)
 * per instance; nk: (K/G) per instance of a problem or NULL; out_norms (G,5).  The caller keeps per-problem rho updates
 * and stopping decisions (ggl_scale_X_batch takes one factor per instance; ggl_get_state_k / ggl_snapshot_k per instance).
 * GGL: K/G <= 32; state exactly symmetric. */
int ggl_mgl_batch_step(ggl_ctx *ctx, int G, const double *rho, const double *lambda1, const double *lambda2,
                       int reg, int latent, const double *mu1, const double *nk, double *out_norms);

/* ---- n iterations of a batch per call (round 5): the HOST LOOP of the grid walks in C -----------------------------------
 * The reference's grid walks (helper/model_selection.py:208-224, :619-633) run, per point and iteration, the stopping test
 * (ADMM_stopping_criterion, solver/admm_solver.py:316-331 / single_admm_solver.py:277-291), the residual-balancing rho rule
 * and the dual rescale (admm_solver.py:227-237 / single_admm_solver.py:196-206).  gglasso_amd.batch did that in NumPy between
 * two C calls (~100 us per batch iteration where the device needs 50 us at p <= 64).
 * ggl_batch_decide (host only, no GPU): one iteration's decisions for n points, bit for bit gglasso_amd.batch._decide --
 *   sq (n,5) squared norms; live (n) 0/1; marked (n) 0/1 or NULL (ggl_failed_instances); rho (n) in/out; dims (n);
 *   last (n,4) {r_t, s_t, e_pri, e_dual} (rows of live finite points rewritten); fac (n) out = rho / rho_new;
 *   status (n) out: 0 goes on, 1 converged now, 2 failed (non-finite sums or marked).  Returns #{status != 0}.
 * ggl_sgl_batch_run / ggl_mgl_batch_run: up to n_iters iterations of ggl_sgl_batch_step / ggl_mgl_batch_step with those
 *   decisions and the X rescale in between.  status (n) in/out: 0 live, 1 converged, 2 failed (points that are not 0 on
 *   entry are dragged along without decisions); last (n,4) in/out; fin_iter (n) in/out: it_base + the iteration of this call
 *   a point finished in (1-based).  snap_ctx NULL: return after the first iteration in which a live point converges or
 *   fails.  snap_ctx given (ctx itself, or the ORIGINAL ctx of a compacted batch; snap_index: destination slot of every
 *   instance slot): a finishing point's whole solution is snapshotted there on the device (ggl_snapshot_state_from), a
 *   failed point is then parked (ggl_reset_instance), and the loop goes on until every point is finished, at least
 *   stop_after points are (> 0: the caller may compact), or n_iters.  Return value: iterations run, < 0 on error.
 * ggl_snapshot_state_from: ggl_snapshot_from + Omega and X; ggl_get_snapshots: the snapshot stacks (K,p,p), any NULL --
 *   ONE download per stack at the end of a batch instead of three or four small ones per point. */
int ggl_batch_decide(int n, const double *sq, const unsigned char *live, const unsigned char *marked, double *rho,
                     const double *dims, double tol, double rtol, int update_rho, double *last, double *fac, int *status);
int ggl_sgl_batch_run(ggl_ctx *ctx, int n_iters, double *rho, const double *lambda1, int latent, const double *mu1,
                      const double *dims, double tol, double rtol, int update_rho, double *last, int *status,
                      int *fin_iter, int it_base, ggl_ctx *snap_ctx, const int *snap_index, int stop_after);
int ggl_mgl_batch_run(ggl_ctx *ctx, int G, int n_iters, double *rho, const double *lambda1, const double *lambda2,
                      int reg, int latent, const double *mu1, const double *nk, const double *dims, double tol, double rtol,
                      int update_rho, double *last, int *status, int *fin_iter, int it_base, ggl_ctx *snap_ctx,
                      const int *snap_index, int stop_after);
int ggl_snapshot_state_from(ggl_ctx *ctx, int k_dst, ggl_ctx *src, int k_src);
int ggl_get_snapshots(ggl_ctx *ctx, double *Omega, double *Theta, double *L, double *X);

/* host only: out = {largest K/G of the batched GGL grid (per-element Theta kernel), largest K of the FGL Theta-step (the
 * K-vectors of a tile of pairs live in LDS)}; callers choose between the batched grid and the sequential walk with it */
int ggl_theta_limits(int out[2]);

/* X <- factor * X : dual rescale after a rho update (admm_solver.py:236). */
int ggl_scale_X(ggl_ctx *ctx, double factor);

/* Exit checks of admm_solver.py:284-301: out = {max|Omega-Omega^T|, max|Theta-Theta^T|,
 * max|L-L^T|, min eig(Theta-L), min eig(L)}. */
int ggl_exit_checks(ggl_ctx *ctx, int latent, double out[5]);

/* The same five numbers per instance, out (K,5) (what the per-instance messages of solver/ext_admm_solver.py:290-311 need). */
int ggl_exit_checks_k(ggl_ctx *ctx, int latent, double *out);
/* The same checks as the DECISIONS the reference takes, without the eigenvalues: out[k*5..] = { the three asymmetries,
 * 1 if Theta_k - L_k - shift_tl I is positive definite else 0, 1 if L_k + shift_l I is positive definite else 0 (1 when not
 * latent) } -- two batched Cholesky factorisations instead of two eigendecompositions.  The reference warns when
 * min eig(Theta - L) <= shift_tl (0 for ADMM_MGL / ADMM_SGL, 1e-5 for ext_ADMM_MGL) resp. min eig(L) < -shift_l (1e-5 / 1e-8):
 * the instances whose flag is 0; ggl_exit_checks_k gives the eigenvalues for the message of a warning that has to be printed. */
int ggl_exit_checks_fast_k(ggl_ctx *ctx, int latent, double shift_tl, double shift_l, double *out);

/* ---- ext_ADMM_MGL: Group Graphical Lasso over instances of DIFFERENT dimension -------------------
 * solver/ext_admm_solver.py:18-323 (loop body :196-231, prox_2norm_G / prox_G_inner :394-453, stopping criterion :325-345,
 * KKT residual :347-392); bookkeeping array G as built by helper/ext_admm_helper.py:104-144, checked like check_G :82-102.
 * Layout: the ctx is created with p = max_k p_k; instance k is the leading (p_k,p_k) block of its (p,p) slot and the
 * caller pads the rest of every stack with an identity block for S, Omega, Theta, Lambda and zeros for the duals (a
 * decoupled fixed point of the iteration; the stopping-test sums skip it).  Omega/Theta/L/X0 travel through
 * ggl_set_state / ggl_get_state (X is X0), Lambda and X1 through ggl_ext_set_state / ggl_ext_get_state.
 *   ggl_ext_setup      pk (K) instance dimensions; G (2,L,K) int32 row-major, -1 = the instance does not hold the pair.
 *                      Every (instance, i, j) may be listed once (GGL_E_ARG otherwise: the groups run in parallel).
 *   ggl_ext_admm_step  one iteration; lambda1 (K) per instance (:133-134), out_norms = the five sums of :325-345:
 *                      |Omega|^2+|Lambda|^2, |Theta-L|^2+|Theta|^2, |X0|^2+|X1|^2, |Omega-Theta+L|^2+|Lambda-Theta|^2,
 *                      |Omega-Omega_prev|^2+|Lambda-Lambda_prev|^2 over all instances (this solver has no rho update).
 *   ggl_ext_kkt_residual  the opt-in stopping_criterion='kkt' of the same solver.  The ctx must hold ONE problem (ggl_ext_setup):
 *                      on a ctx set up with ggl_ext_setup_batch it returns GGL_E_ARG before anything is launched. */
int ggl_ext_setup(ggl_ctx *ctx, const int *pk, const int *G, int L);
int ggl_ext_set_state(ggl_ctx *ctx, const double *Lambda, const double *X1);
int ggl_ext_get_state(ggl_ctx *ctx, double *Lambda, double *X1);
int ggl_ext_admm_step(ggl_ctx *ctx, double rho, const double *lambda1K, double lambda2, int latent,
                      const double *mu1, double out_norms[5]);
int ggl_ext_kkt_residual(ggl_ctx *ctx, double rho, const double *lambda1K, double lambda2, int latent,
                         const double *mu1, double *out);
/* nprob independent ext_ADMM_MGL problems with the SAME instance dimensions and bookkeeping array in one ctx -- the
 * (lambda1, lambda2) points the MAIN LOOP of grid_search (helper/model_selection.py:208-224) hands to ext_ADMM_MGL one after
 * the other: the ctx stack holds nprob * K instances, problem g in the slots g*K .. (the caller replicates the padded S).
 *   ggl_ext_setup_batch  pk (K) and G (2,L,K) of ONE problem
 *   ggl_ext_batch_step   one iteration of all problems: lambda1 (nprob*K) per instance slot, lambda2 (nprob) per problem, one
 *                        rho (this solver has no rho update), mu1 (nprob*K); out_norms (nprob,5): the five sums per problem.
 * The caller keeps the stopping decision per problem (ggl_get_state_k / ggl_ext_get_state per instance slot). */
int ggl_ext_setup_batch(ggl_ctx *ctx, int nprob, const int *pk, const int *G, int L);
int ggl_ext_batch_step(ggl_ctx *ctx, double rho, const double *lambda1K, const double *lambda2G, int latent,
                       const double *mu1, double *out_norms);

/* Model selection over a batch of independent problems (reference: single_grid_search,
 * helper/model_selection.py:505-692; criteria :812-856; robust_logdet :884-894).
 * ggl_snapshot_k keeps a device copy of instance k's Theta at the moment the host loop declares it converged;
 * ggl_selection_stats then returns, for every instance's snapshot,
 * out[k*4..] = { <S_k,Theta_k>, log det Theta_k (-inf if lambda_min <= 1e-12), count_nonzero(Theta_k),
 * lambda_min(Theta_k) }.  After a latent step ggl_snapshot_k keeps L_k as well.
 *
 * ggl_threshold_scan: tune_threshold (helper/model_selection.py:707-737, thresholding :698-705) for every snapshot at
 * once: out[(k*ntau + j)*4..] = the same four numbers for T = Theta_k with the off-diagonal entries |t| <= tau[j]
 * zeroed.  Thresholds that zero the same entries of an instance give the same matrix; only the distinct ones go
 * through the eigenvalue kernel (*n_eig = how many, may be NULL).
 *
 * ggl_selection_rank: numpy.linalg.matrix_rank of every L_k snapshot (model_selection.py:256, :638):
 * out[k*4..] = { #{|lambda_i| > rel_tol * max|lambda|}, max|lambda|, largest |lambda| not counted, smallest |lambda|
 * counted }; rel_tol <= 0: numpy's p*eps.  The two neighbours of the cut let the caller see how clear the decision
 * was: the null space of an L that came out of the sign-iteration L-step (p > GGL_JACOBI_MAX_P) carries that
 * iteration's residual (~1e-12 |L|), far above numpy's tolerance but far below any eigenvalue the prox keeps. */
int ggl_snapshot_k(ggl_ctx *ctx, int k);
/* the same from another ctx of the same dimension (a compacted batch, ggl_ctx_create_subset): instance ks of src into slot kd */
int ggl_snapshot_from(ggl_ctx *ctx, int kd, ggl_ctx *src, int ks);
int ggl_selection_stats(ggl_ctx *ctx, double *out);
int ggl_threshold_scan(ggl_ctx *ctx, const double *tau, int ntau, double *out, int *n_eig);
int ggl_selection_rank(ggl_ctx *ctx, double rel_tol, double *out);
/* The latent component a solve RETURNS (reference: prox_rank_norm, solver/ggl_helper.py:29-36, as the last L-step of
 * admm_solver.py:197-205 / single_admm_solver.py:172-175 leaves it: Q diag(max(d - mu1/rho, 0)) Q^T, null space exact to
 * rounding -- the reference's callers apply numpy.linalg.matrix_rank to it, helper/model_selection.py:254, :638).
 * Above GGL_JACOBI_MAX_P the per-iteration L-step is the sign iteration, whose L is entrywise right to ~1e-13 |L| but whose
 * null space carries that residual.  ggl_finalize_L rebuilds L from ONE eigendecomposition of the last L-step's input
 * C = Theta - X - Omega (kept on the device by the step itself / by ggl_snapshot_k) -- the reference's own L-step, run
 * once per solve instead of once per iteration.  X is left as the last dual update wrote it.
 *   which 0: the live iterate's L (call before ggl_get_state / ggl_exit_checks);  1: the L snapshots of ggl_snapshot_k
 *   rank_out (K ints, may be NULL): #{ eigenvalues of C_k above mu1_k/rho } for every rebuilt instance, -1 otherwise
 * Returns the number of instances rebuilt -- 0 when every L already is an eigendecomposition's (p <= GGL_JACOBI_MAX_P,
 * GGL_OPT_RANK_EIG, a fallback in the last step, an uploaded L) and nothing was done -- or an error code < 0.
 * ggl_get_snapshot_k: Theta and L (either may be NULL) of instance k's snapshot. */
int ggl_finalize_L(ggl_ctx *ctx, int which, int *rank_out);
/* Fault isolation and compaction of a batch of independent problems (the reference's grid walk, helper/model_selection.py:
 * 208-224, solves its points one by one: a point that fails costs that point, a point that has converged costs nothing more).
 *   GGL_OPT_ISOLATE       see above; ggl_failed_instances: out[k] = 1 for every instance marked so far (out may be NULL),
 *                         returns their number
 *   ggl_reset_instance    parks instance k on the identity problem (S = Omega = Theta = I, L = X = 0): finite, cheapest schedules
 *   ggl_ctx_create_subset a new ctx with the m instances idx[] of src (S, iterate, masks, dimensions, options; device to
 *                         device), for the points still iterating once a good part of the batch is done; src stays valid */
/* Debugging aid, process-wide: after ggl_debug_poison(1) every ctx created fills its device and pinned buffers with 0xFF bytes
 * (NaN doubles, -1 ints) instead of zeros before it initialises what it documents as initialised -- a read of memory the library
 * never wrote then fails at once instead of depending on what an earlier allocation left behind.  2..255: that byte instead
 * (0x7F: 1.4e306, 0x47: 1.5e35 -- finite garbage, which a max / min reduction or a comparison keeps where it drops a NaN).
 * tests/conftest.py switches it on for a whole session when GGL_DEBUG_POISON=<n> is set in the environment of the TEST process. */
int ggl_debug_poison(int on);
/* Process-wide switch: odd p on the direct-to-LDS product kernel (1, default since round 6) or on the register-staged kernel as
 * in rounds 1-5 (0); returns the previous setting.  Same products either way (parity test of the two routes, A/B runs). */
int ggl_set_odd_dl(int on);
int ggl_failed_instances(ggl_ctx *ctx, int *out);
/* Why instance k was marked (the first mark stays): out[0] = 1 a spectral or norm bound that was not finite or not positive,
 * 2 an eigensolver that did not converge, 3 a non-finite residual or trace in the L-step's sign iteration, 4 marked inside a
 * fused batch iteration, 0 not marked; out[1] = the offending value (the bound, the solver's info, the residual).  What the
 * batch drivers put into the warning that goes with a 'solver error' point. */
int ggl_failed_reason(ggl_ctx *ctx, int k, double out[2]);
int ggl_reset_instance(ggl_ctx *ctx, int k);
int ggl_ctx_create_subset(ggl_ctx *src, const int *idx, int m, ggl_ctx **out);
int ggl_get_snapshot_k(ggl_ctx *ctx, int k, double *Theta, double *L);
/* Omega and X of instance k's snapshot (ggl_snapshot_state_from), either may be NULL: what a grid walk fetches for the ONE point it
 * selects after it has taken Theta (and L) of all points with ggl_get_snapshots(NULL, Theta, L, NULL) -- the reference's
 * single_grid_search returns the whole sol of the best point only (helper/model_selection.py:652-660). */
int ggl_get_snapshot_state_k(ggl_ctx *ctx, int k, double *Omega, double *X);
/* Objective pieces for measure=True (admm_solver.py:213): out = {sum_k -logdet Omega_k,
 * <Omega,S>, P_val(Theta)} (ggl_helper.py:266-270,162-176). */
int ggl_objective(ggl_ctx *ctx, double lambda1, double lambda2, int reg, double out[3]);

/* KKT residual of admm_solver.py:333-371 / single_admm_solver.py:293-320 on the ctx state
 * (opt-in stopping_criterion='kkt').  The dual passed by the reference is rho*X. */
int ggl_kkt_residual(ggl_ctx *ctx, double rho, double lambda1, double lambda2, int reg, int latent,
                     const double *mu1, const double *nk, double *out);
/* The four terms ggl_kkt_residual is the maximum of, in the reference's order (admm_solver.py:343-371,
 * single_admm_solver.py:302-317): |Theta - prox(Theta + rho X)| / (1 + |Theta|), |Theta - Omega - L| / (1 + |Theta|),
 * |Omega - phiplus(Omega - nk S - rho X)| / (1 + |Omega|), |L - prox_rank(L - rho X, mu1)| / (1 + |L|) (0 when not latent).
 * GGL_REG_SGL thresholds instance k with lambda1, with the shared mask of ggl_set_lambda1_mask or with its own array of
 * ggl_set_lambda1_mask_k, as the step does.  Same launches in the same order as ggl_kkt_residual, same refusals. */
int ggl_kkt_terms(ggl_ctx *ctx, double rho, double lambda1, double lambda2, int reg, int latent,
                  const double *mu1, const double *nk, double out[4]);
/* What the diagnostics dispatched on this ctx since it was created: out = { ggl_objective calls whose log det came from the
 * eigenvalues of W the last Omega-step left, from the Cholesky factor of Omega, from the eigenvalues of Omega behind a failed
 * factorisation; KKT calls (ggl_kkt_terms / ggl_kkt_residual) on the LDS Jacobi eigensolver, on rocSOLVER, with the shared
 * lambda1 mask, with per-instance masks; 0 }. */
int ggl_diag_stats(ggl_ctx *ctx, long long out[8]);

/* ---- per-phase device timing (HIP events on the ctx stream; what bench.py's roofline uses) ------
 * Phases of one iteration; ms[] accumulates elapsed milliseconds, count[] the number of launches. */
#define GGL_PH_FORM_W 0       /* W = Theta - L - X - (nk/rho) S                                  */
#define GGL_PH_EIG_OMEGA 1    /* eigensolver of the Omega-step (LDS Jacobi: includes phiplus)     */
#define GGL_PH_RECON_OMEGA 2  /* Q phip(D) Q^T reconstruction (FP64 MFMA)                          */
#define GGL_PH_THETA 3        /* Theta-step (+ fused dual update and norms when not latent)       */
#define GGL_PH_EIG_L 4        /* eigensolver of the L-step                                        */
#define GGL_PH_RECON_L 5      /* Q max(D-mu,0) Q^T                                                 */
#define GGL_PH_DUAL 6         /* X += Omega - Theta + L and norms (latent path)                   */
#define GGL_PH_REDUCE 7       /* partial-sum reduction of the norms                                */
#define GGL_PH_EIG_OMEGA2 8   /* second part of the Newton-Schulz Omega-step (after the spectral-bound sync) */
#define GGL_PH_BOUND 9        /* (not recorded any more: the bound kernels run inside the Omega-step chains) */
#define GGL_PH_ALLREDUCE_GROUPSQ 10 /* K-sharded run: ncclAllReduce of the p(p+1)/2 + 1 packed group sums (ggl_admm_step_sharded)  */
#define GGL_PH_ALLREDUCE_NORMS 11   /* K-sharded run: ncclAllReduce of the five sums                                    */
#define GGL_NPHASE 12
/* on: 0 off, 1 every phase, 2 only GGL_PH_EIG_OMEGA / _OMEGA2 / _EIG_L and the two all-reduces (4-10 event records per iteration) */
int ggl_profile_enable(ggl_ctx *ctx, int on);
int ggl_profile_read(ggl_ctx *ctx, double ms[GGL_NPHASE], long long count[GGL_NPHASE], int reset);
/* Newton-Schulz statistics since ctx creation: Omega-step {calls, steps, calls that took the stable
 * schedule, algorithmic work in units of K*p^3 flop, kernel launches}; L-step {calls, retries at the
 * finer resolution, fallbacks to the eigendecomposition, kernel launches in units of K*p^3 flop (a launch on a compact
 * sub-batch of m instances counts m/K)}; speculative
 * Omega-steps {taken, failed validation and repeated}; [11] end-of-iteration polls that timed out and fell back to a
 * stream synchronisation; what the LAST matrix-function step dispatched: [12] concurrent parts, [13] product-kernel
 * variant (csrc/gemm_sym.hip); [14] Omega-steps that fell back to the eigendecomposition; [15] pre-launched Omega-step
 * chains (GGL_OPT_PIPELINE) that were dropped unused. */
int ggl_ns_stats(ggl_ctx *ctx, long long out[16]);
/* The LDS-resident Omega-step (GGL_OPT_OMEGA_LDS): out = { launches, launches repeated on the launch chain because an instance
 * fell outside the kernel's range, products summed over all instances of all launches, Newton-Schulz steps likewise }. */
int ggl_lds_stats(ggl_ctx *ctx, long long out[4]);
/* GGL_OPT_GROUP_SCHED: out = { Omega-steps that ran as groups with their own schedules, groups of the last step (1 = whole batch),
 * lengths of its groups [4], product units (A', B' included) of their schedules [4], grouped steps whose split differed from
 * the previous grouped step's }; units_sum (4 doubles, may be NULL): the units of every group slot summed over the grouped steps. */
int ggl_group_stats(ggl_ctx *ctx, long long out[11], double *units_sum);
/* GGL_OPT_OMEGA_POLY: out = { launch sequences of the Omega-step that ran the direct family, launch sequences in all (concurrent
 * parts and groups count one each), degree of the last direct polynomial }. */
int ggl_omega_poly_stats(ggl_ctx *ctx, long long out[3]);
/* c_k >= lambda_max(W_k^2 + 4 beta_k I) and beta_k (K doubles each) of the last validated matrix-function Omega-step; returns 1,
 * or 0 when there is none yet. */
int ggl_spectral_bounds(ggl_ctx *ctx, double *c_out, double *beta_out);
/* Pipelining across iterations (GGL_OPT_PIPELINE, ggl_admm_step): out = { whole Omega-step chains launched ahead of the caller's
 * next step (after an iteration was validated, while the caller looks at its residuals), of those forgotten because rho changed,
 * early first parts (tables, W, A', B' of the NEXT iteration's chain, put into the stream before the host waits for this
 * iteration's residuals), of those continued, fresh streams the concurrency probe had to try before the first two-part
 * Omega-step until one ran BESIDE the ctx's main stream (HIP streams share a small pool of hardware queues, and two streams on
 * one queue serialise; 0: the part stream was fine, -1: not probed yet), Theta-steps that also wrote the next Omega-step's W
 * (GGL_OPT_FUSED_W), of those used by the early first part that followed, bound validations that rode in a product launch
 * (GGL_OPT_CW_RIDER; counted per part), table transfers that rode in an A' launch (GGL_OPT_COPY_RIDER; per part), norm
 * reductions that did (GGL_OPT_REDUCE_RIDER) }. */
int ggl_pipeline_stats(ggl_ctx *ctx, long long out[10]);
/* L-step (sign iteration): out = { calls, calls whose first pass was continued on a compact sub-batch, instances continued in
 * total, calls that fell back to the eigendecomposition } */
int ggl_rank_stats(ggl_ctx *ctx, long long out[4]);
/* out = { L-step calls whose first pass was followed by the deflation, instances that had directions to deflate } */
int ggl_deflate_stats(ggl_ctx *ctx, long long out[2]);
/* ggl_finalize_L checks its eigendecomposition (the eigenvalues of every rebuilt instance add up to the trace of its L-step input,
 * taken before the eigensolver overwrites it) and repeats it once on a kept copy if they do not: out = { eigendecompositions
 * run, of those repeated }. */
int ggl_finalize_stats(ggl_ctx *ctx, long long out[2]);
/* What ran last: out = { concurrent parts and product-kernel variant of the last matrix-function step (as in ggl_ns_stats),
 * code of the Theta kernel of the process's last Theta-step (0 GGL tile pairs; 100+KMAX per-element kernel with the K-column
 * in one thread; 100*KQ+NW per-element kernel with the K-column over NW waves: 404, 408, 808, 816, 1616; 2000+tile FGL
 * Condat tiles), eigendecompositions ggl_finalize_L ran on this ctx }.  The parity tests assert the dispatch with it. */
int ggl_last_dispatch(ggl_ctx *ctx, long long out[4]);
/* Functional SGL (ggl_set_block_size): out = { block size M (0 = none), Theta-steps that ran as ONE launch over tile pairs
 * (M <= 32; ggl_last_dispatch reports 4000 + tile edge), Theta-steps behind the table of block sums (M > 32; 5000 + tile edge),
 * fused one-launch SGL iterations (p <= 64, element-wise shrink) this ctx ran -- 0 for as long as a block size was set }. */
int ggl_fsgl_stats(ggl_ctx *ctx, long long out[4]);
/* Event timeline of ggl_admm_step's iterations without a profiler (round 5; tools/event_timeline.py): after ggl_trace_start every
 * launch of the iteration is followed by an event on its stream and the host notes its own marks; ggl_trace_read stops the
 * recording and returns rows {kind 0 device / 1 host, lane (0 main stream, 1.. part streams; -1 host), tag, microseconds since the
 * start}.  Device rows give the COMPLETION time of the launch they follow.  Device tags: 1 parameter copy, 2 form_W, 3 bound_rows,
 * 4 cw_final, 10 product, 11 pair of products, 20 Theta-step, 21 norm reduction; host tags: 100 step entered, 101 Theta-step and
 * reduction queued, 102 early first part queued, 103 residuals seen, 104 rest of the next chain queued (the step returns).
 * ggl_set_S_from_weighted adds the device tags 30 (weights prepared, means done) and 31 (its Gram kernel done). */
int ggl_trace_start(ggl_ctx *ctx, int max_events);
int ggl_trace_read(ggl_ctx *ctx, double *out, int cap);
/* per-instance status of the last eigensolver launch a step fetched: sweeps of the LDS Jacobi kernel (-1: not converged) or
 * rocSOLVER's info */
int ggl_eig_info(ggl_ctx *ctx, int *out);

/* ---- kernel-level test / measurement entry points (not used by the solvers) --------------------
 * ggl_dev_symm: one launch of the symmetric-product kernel on host data (kernel unit test; variant < 0 = by size).
 * ggl_dev_symm_bench: average milliseconds of `iters` launches on random device data (HIP events).
 * Both return GGL_E_ARG for a variant that is not in this build. */
int ggl_dev_symm(int K, int p, const double *A, const double *B, const double *E, const double *coef5K,
                 double *C, double *C2, int variant);
int ggl_dev_symm_bench(int K, int p, int variant, int iters, double *ms_out);
/* ggl_dev_omega_lds: the Omega-step of small matrices (p <= 64) as ONE launch, one workgroup per instance, the Newton-Schulz
 * chain resident in LDS, bound and schedule chosen on the device (omega_lds.hip; kernel unit test and timing).
 * Omega = phiplus(Theta - L - X - beta S, beta), L may be NULL.  cbound (K) or NULL receives the bound used.
 * out[14] = {ms per launch, fallback flag, products summed over the instances, entries of the schedule table, [4..12] phase
 * stamps of instance 0 in us (start, W, A', B', bound, first step, steps, W again, Omega), [13] products of instance 0}.
 * degrees + 1000 * w: w = 4 or 8 waves per workgroup (0: by size, as the solver runs it). */
int ggl_dev_omega_lds(int K, int p, const double *Theta, const double *L, const double *X, const double *S, const double *beta,
                      double tol, int degrees, double *Omega, double *cbound, int iters, double *out);
/* ggl_dev_symm_bounds: C = A B on the direct-to-LDS product kernel with the bound partials of its epilogue, reduced to
 * the row sums of |C| (K,p), |C|_F^2 (K) and the spectral bound sqrt(min(|C|_inf, Collatz-Wielandt ratio, |C|_F)) (K)
 * that the Omega-step takes from B' = (W^2 + 4 beta I)^2 (kernel unit test; even p, variants 16 / 17 / 20). */
int ggl_dev_symm_bounds(int K, int p, const double *A, const double *B, int variant, double *C,
                        double *rowsum_out, double *fro2_out, double *bound_out);
/* host only (no GPU needed): the Newton-Schulz step schedule the Omega-step would run for a spectrum in [l,1]
 * (x = sqrt(eig(Z Y))).  degrees 3 = cubic steps, 5 = cubic/quintic mix, 9 = cubic/quintic/degree-nine mix.
 * deg_out[max_steps] receives 3, 5 or 9 per step, coef_out[max_steps*6] = {t0..t4,l_after} of
 * x -> x (t0 + t1 x^2 + ... + t4 x^8), *units_out the number of
 * symmetric products of the stack (incl. A' and B').  degrees + 100: the schedule of the L-step's sign iteration
 * instead (every step costs X^2, [t], X t: 2 / 3 / 4 products; *units_out without the first and the last product).
 * Returns the number of steps or GGL_E_ARG. */
int ggl_dev_ns_schedule(double l, int degrees, int max_steps, int *deg_out, double *coef_out, int *units_out);
/* the same for the Omega-step at a stopping tolerance (GGL_OPT_NS_TOL; 0 = fp64 resolution, what the call above plans for) */
int ggl_dev_ns_schedule_tol(double l, int degrees, double tol, int max_steps, int *deg_out, double *coef_out,
                            int *units_out);
/* host only: the grouping rule of GGL_OPT_GROUP_SCHED -- units[k] = product count of instance k's schedule; returns the number of
 * contiguous groups (1 = whole) and their lengths in len_out[3] -- and the product count (A', B' included) of the all-symmetric
 * schedule for a spectrum in [l, 1] at the stopping tolerance tol (-1: condition number above 300, the stable schedule's range) */
int ggl_dev_group_partition(const int *units, int K, int p, int max_groups, int *len_out);
int ggl_dev_ns_units(double l, int degrees, double tol);
/* host only: the direct family of the Omega-step (GGL_OPT_OMEGA_POLY) for the spectral interval [a, 1] of A'/c: out[18] = the
 * monomial coefficients [16] of p in X = (A'/c - m I)/h, m = (1+a)/2, h = (1-a)/2, for the quantised a (out[16]; rounded down),
 * and p's certified relative deviation from sqrt(m + h X) (out[17]); *deg = its degree (6, 9, 12, 15; 0 = none meets tol),
 * *units = its products, A' and B' included (-1: none).  Returns 1 where an Omega-step launch sequence with this interval takes
 * the direct family -- strictly fewer products than the Newton-Schulz schedule of (degrees, tol) -- and 0 where it does not. */
int ggl_dev_omega_poly_plan(double a, double tol, int degrees, int *deg, double *out, int *units);
#ifdef GGL_DEV
/* C = A B on the INT8 matrix cores from S signed-digit slices per operand (error-free split; gemm_i8.hip), slice pairs
 * t + u <= dmax; |A| <= scaleA, |B| <= scaleB entrywise.  ms_out = {slicing both operands, one product launch, overflow flag}. */
int ggl_dev_i8_stages(int n);   /* LDS stages of the int8 product kernel: 1 (default) or 2 */
int ggl_dev_symm_i8(int K, int p, int S, int dmax, const double *A, const double *B, double scaleA, double scaleB, double *C,
                    int iters, double *ms_out);
/* The whole Omega-step phiplus(W) (solver/ggl_helper.py:272-303) on the int8 matrix cores, stand-alone: W (K,p,p), beta (K),
 * cbound (K) >= lambda_max(W^2 + 4 beta I); cfg5 = {slices of the full products, of F F, of G F^2, of Y E, diagonal cut of Y E}
 * or NULL; tol: the schedule's stopping tolerance.  ms_out = {ms per step, product launches, overflow flag, fp64 products the
 * schedule stands for}. */
int ggl_dev_omega_i8(int K, int p, const double *W, const double *beta, const double *cbound, const int *cfg5, double tol,
                     double *Omega, int iters, double *ms_out);
/* libggl_hip_dev.so only (python -m gglasso_amd.build --dev): measured FP64 matrix-core ceiling of this GPU in TFLOP/s
 * (MFMA-only probe kernel); per-workgroup timestamps {start, loop begin, loop end, end, XCC id} of one launch of the
 * 64x64 kernel */
int ggl_dev_mfma_f64_peak(double *tflops_out);
/* FP64 VALU || FP64 MFMA co-issue probe (csrc/probes_dev.hip), TF/s: {MFMA only, v_fma_f64 only, waves split per SIMD:
 * MFMA, DFMA, one wave with 4 / 8 / 16 / 32 v_fma_f64 behind every MFMA: MFMA, DFMA each} */
int ggl_dev_coissue_probe(double *out12);
/* MFMA fed from LDS (the product kernel's inner loop alone), TF/s for wave tiles {2x2 @3 WG/CU, 2x2 @5, 2x4 @3, 4x4 @2, 4x4 @3, 1x1 @5} */
int ggl_dev_mfma_lds_probe(double *out6);
/* What a change of kernel between dependent launches costs (tools/kernel_switch_cost.py): mode 0 `iters` product launches, 1 each
 * followed by a one-thread kernel, 2 the one-thread kernel alone, 3 each followed by an elementwise kernel over its output;
 * ms per repetition. */
int ggl_dev_switch_bench(int K, int p, int variant, int iters, int mode, double *ms_out);
/* A measured ceiling for the product kernel: the vendor's FP64 GEMM at the same shapes (tools/bench_vendor.py).  mode 0
 * rocblas_dgemm_strided_batched (N,N), 1 (T,N), 2 rocblas_dsyrk_strided_batched (one triangle), 3 rocblas_dsyrkx_strided_batched
 * (one triangle of A B^T: the library's form of a symmetric product), 4 the product kernel itself.  ms per call. */
int ggl_dev_vendor_bench(int K, int p, int mode, int iters, double *ms_out);
/* Probe for reading (A) of round 5's intermittent RANK table: hipMalloc + hipMemsetAsync of a (K,p,p) stack and
 * hipMemcpyAsync device-to-device copies of `slices` instances into it on one stream, `reps` times; out = { repetitions, slices
 * that came out zero }. */
int ggl_dev_fill_copy_probe(int reps, int K, int p, int slices, int gap_us, long long out[2]);
int ggl_dev_symm_timeline(int K, int p, long long *out, int max_blocks, int *nblocks_out);
/* Epilogue of the direct-to-LDS product kernels (symm_dl_tile): 0 the batched one that writes off-diagonal tiles and their
 * mirrors from registers (the only one the product library has), 1 the serial one, kept as its bitwise yardstick and for A/B
 * timing, 2 the batched one with every off-diagonal tile staged in LDS (the product's before the register path).  Any other
 * value counts as 0.  Process-wide; returns the previous mode. */
int ggl_dev_set_symm_epilogue(int mode);
/* ggl_dev_symm_bench with the epilogue's operands present: ops bit 0 the affine operand E, bit 1 the second one (E2), bit 2 the
 * second output C2.  Average milliseconds of `iters` launches. */
int ggl_dev_symm_bench_ops(int K, int p, int variant, int iters, int ops, double *ms_out);
/* ggl_dev_symm with every operand of the epilogue: E and E2 (either may be NULL), the full coefficient rows coef8K (K x 8:
 * cI, cAcc, cE, dI, dC, dE, cE2, dE2) and the second output C2 (may be NULL). */
int ggl_dev_symm_full(int K, int p, const double *A, const double *B, const double *E, const double *E2, const double *coef8K,
                      double *C, double *C2, int variant);
#endif

/* ---- stateless operator entry points (host buffers; used for operator-level parity) ---------- */
/* numpy.linalg.eigh on a stack (lower triangle read); D (K,p) ascending, Q (K,p,p) columns. */
int ggl_eigh_batched(int K, int p, const double *A, double *D, double *Q, int eig_method);
/* phiplus(beta,D,Q), ggl_helper.py:280-303, for K matrices; beta (K,). */
int ggl_phiplus(int K, int p, const double *beta, const double *D, const double *Q, double *out);
/* prox_rank_norm(A,beta,D,Q), ggl_helper.py:29-36. */
int ggl_prox_rank_norm(int K, int p, const double *beta, const double *D, const double *Q, double *out);
/* eigh + phiplus / rank shrink fused, straight from the matrix (what the ADMM step runs). */
int ggl_phiplus_matrix(int K, int p, const double *beta, const double *W, double *out, int eig_method);
int ggl_rank_matrix(int K, int p, const double *beta, const double *C, double *out, int eig_method);
/* the same with the two-tier control of the sign-iteration L-step exposed: l0_coarse as GGL_OPT_RANK_L0_COARSE (< 0: the default),
 * stats (may be NULL) = { calls, calls continued on a compact sub-batch, instances continued, eigendecomposition fallbacks,
 * retries of the whole batch, product launches } */
int ggl_rank_matrix_ex(int K, int p, const double *beta, const double *C, double *out, int eig_method, double l0_coarse,
                       long long stats[6]);
/* the same with the DEFLATING L-step (a first pass at l0_deflate, <= 0: the default GGL_OPT_RANK_L0_DEFLATE, then the
 * eigenvalues next to the threshold as the range of I - X^2; csrc/deflate.hip); ggl_rank_matrix_ex with l0_coarse >= 0 runs
 * the two-tier iteration without it.  stats[8] = the six above + { calls followed by the deflation, instances deflated } */
int ggl_rank_matrix_deflate(int K, int p, const double *beta, const double *C, double *out, int eig_method, double l0_deflate,
                            long long stats[8]);
/* prox_od_1norm(A,l), ggl_helper.py:16-27; lam_pp NULL => scalar lam. */
int ggl_prox_od_1norm(int p, const double *A, double lam, const double *lam_pp, double *out);
/* prox_sum_Frob(X,M,l), ggl_helper.py:45-66: X, out (p,p), M divides p.  The upper blocks decide; the lower triangle of X
 * is read on the diagonal blocks only. */
int ggl_prox_sum_frob(int p, int M, const double *X, double l, double *out);
/* frob_norm_per_block(S,M,off_diag), helper/utils.py:69-87: out (p/M,p/M), Frobenius norm of every M x M block (upper blocks
 * mirrored), diagonal 0 when off_diag; lambda_max_fsgl (helper/utils.py:89-107) is the maximum of that table. */
int ggl_frob_norm_per_block(int p, int M, const double *S, int off_diag, double *out);
/* prox_p(X,l1,l2,reg), ggl_helper.py:190-207 (reg = GGL_REG_GGL | GGL_REG_FGL). */
int ggl_prox_p(int K, int p, const double *X, double l1, double l2, int reg, double *out);
/* n independent K-vectors, Y (n,K) row-major: prox_tv = condat_method (fgl_helper.py:11-68),
 * prox_2norm (ggl_helper.py:38-43), prox_phi_ggl / prox_phi_fgl. */
int ggl_prox_tv(int n, int K, const double *Y, double lam, double *out);
int ggl_prox_2norm(int n, int K, const double *Y, double lam, double *out);
int ggl_prox_phi(int n, int K, const double *Y, double l1, double l2, int reg, double *out);

/* ---- sample covariance from data, scaling by a diagonal (covariance.hip) ----------------------------------------------
 * flags of ggl_covariance / ggl_set_S_from_data */
#define GGL_COV_CENTER 1    /* subtract the row means (off: the raw second moment) */
#define GGL_COV_SCALE 2     /* also scale to correlations; scale_out gets the variances */
#define GGL_COV_TILE32 4    /* tile choice of the Gram kernel forced to 32 x 32 / 64 x 64 (tests, measurements); */
#define GGL_COV_TILE64 8    /* default: 64 x 64 where K T (T + 1) / 2 tile pairs fill the chip, else 32 x 32 */
/* numpy.cov(X_k, bias=True) per instance (helper/data_generation.py:221,234): X_host[k] is the row-major (p, N[k]) array of
 * instance k, variables in rows; S_out (K,p,p), exactly symmetric; scale_out (K,p) or NULL (needed with GGL_COV_SCALE).
 * Fixed reduction orders: two calls give bitwise equal results, instance k's result does not depend on the others.
 * GGL_COV_SCALE with a variable of zero (or non-finite) variance is GGL_E_ARG, naming instance and variable. */
int ggl_covariance(int device, int K, int p, const int *N, const double *const *X_host, int flags, double *S_out,
                   double *scale_out);
/* scale_array_by_diagonal (helper/basic_linalg.py:46-65): Y[k,i,j] = X[k,i,j] / (sqrt(d[k,i]) sqrt(d[k,j])), X, Y (K,p,p);
 * d_in (K,p), or NULL = diag(X), which d_out (K,p, may be NULL) then returns.  A d <= 0 or non-finite is GGL_E_ARG (the
 * reference returns NaN / inf silently), naming instance and variable; nothing is written then. */
int ggl_scale_by_diagonal(int device, int K, int p, const double *X_host, const double *d_in, double *Y_out, double *d_out);
/* The S of a ctx computed on the device from data and left there (no upload of S, no round trip); ctxs without instance
 * dimensions (ggl_set_instance_dims).  Like ggl_set_S it forgets what earlier iterations carried. */
int ggl_set_S_from_data(ggl_ctx *ctx, const double *const *X_host, const int *N, int flags);
/* S_out (K,p,p); scale_out (K,p): the variances, NULL unless the ctx's S came from data with GGL_COV_SCALE */
int ggl_get_S(ggl_ctx *ctx, double *S_out, double *scale_out);

/* ---- StARS stability selection from data (Liu, Roeder, Wasserman 2010): both ends of a batch of B subsamples x L lambdas
 * on the device (stars.hip).  Entry points that are only ADDED: GGL_VERSION stays where it is.
 *
 * Covariances of B column subsets of ONE data array: X_host the row-major (p,N) array, variables in rows, idx the (B,b)
 * int array of sample indices in [0,N) (duplicates allowed: a bootstrap draw; any order).  X goes up once, the columns are
 * gathered on the device, and subset r's matrix is bitwise what the covariance call above returns for the gathered (p,b) array
 * in a call of K = B instances.  S_out (B,p,p), scale_out (B,p) or NULL, flags as above.  GGL_E_ARG, found before any device
 * work: an index outside [0,N) (the message names subset and position), b < 1, B < 1. */
int ggl_covariance_subsets(int device, int p, int N, const double *X_host, int B, int b, const int *idx, int flags,
                           double *S_out, double *scale_out);
/* ... straight into the S of a ctx whose K is a multiple of B: instance k gets subset k % B (the layout of the S upload
 * with period B), replicated on the device.  Bookkeeping as the data call above (what earlier iterations carried is forgotten,
 * the variances are kept with GGL_COV_SCALE); a refused call leaves the ctx's S as it was. */
int ggl_set_S_from_subsets(ggl_ctx *ctx, const double *X_host, int N, int B, int b, const int *idx, int flags);
/* Edge stability over the Theta snapshots of a ctx with K = L * B instances, instance l * B + r = subsample r at lambda l:
 * c[l,i,j] = #{ r : |Theta[l*B+r,i,j]| >= t } for i < j (a NaN is no edge; only the upper triangle of a Theta is read),
 * num_out[l] = sum_{i<j} c (B - c), an exact integer (L values); counts_out (L,p,p) int32 or NULL: c mirrored, zero diagonal.
 * Integer sums: two calls return the same bits.  GGL_E_ARG: B < 1 or not dividing K, t negative or not finite, no snapshot. */
int ggl_edge_stability(ggl_ctx *ctx, int B, double t, int *counts_out, long long *num_out);

/* ---- K-fold cross-validation of lambda1 from data: the held-out score of every solution, on the device (k_heldout_dot,
 * stars.hip).  An entry point that is only ADDED: GGL_VERSION stays where it is.
 *
 * For a ctx of K = L * F instances that holds Theta snapshots, instance k = fold k % F at lambda k / F (the layout of
 * ggl_set_S_from_subsets with B = F).  idx_test (F,m): the observations fold f was NOT fitted on.  The F test covariances are
 * bitwise what ggl_covariance_subsets returns for (X_host, idx_test, flags); they live in a temporary device stack, the
 * ctx's S is neither read nor written.
 *   out[k*4..] = { <S_test[k % F], Theta_k>, log det Theta_k, count_nonzero(Theta_k), lambda_min(Theta_k) }
 * the last three the bits of ggl_selection_stats.  The inner product is summed in a fixed order without floating-point
 * atomics: two calls return the same bits, and instance k's value depends on Theta_k and S_test[k % F] alone.
 * flags: GGL_COV_CENTER or 0.  GGL_E_ARG, found before any device work (nothing is written to out, the ctx stays as it
 * was): any other flag bit, F < 1 or not dividing K, m < 1, an index outside [0,N) (the message names fold and position),
 * a NULL buffer, a ctx without snapshots, a ctx with instance dimensions. */
int ggl_heldout_scores(ggl_ctx *ctx, const double *X_host, int N, int F, int m, const int *idx_test, int flags,
                       double *out);

/* ---- Rank correlation from data: Kendall's tau-b between every pair of variables and the nonparanormal skeptic matrix
 * sin(pi/2 tau) (Liu, Han, Yuan, Lafferty, Wasserman 2012) on the int8 matrix cores (kendall.hip).  Entry points that are only
 * ADDED: GGL_VERSION stays where it is.
 *
 * ranks_host: the row-major (p,N) int array of DENSE ranks of every variable (equal values, equal ranks; every entry in
 * [0,N)), variables in rows.  idx: the (B,b) int array of sample indices in [0,N) of B subsets (duplicates allowed: they
 * form tied pairs; any order), or NULL = all N samples as one subset (B = 1, b = N).
 * G_out (B,p,p) 64-bit integers: G[r,i,j] = sum over the pairs a < b of positions of subset r of
 * sgn(R[i,idx[r,a]] - R[i,idx[r,b]]) * sgn(R[j,idx[r,a]] - R[j,idx[r,b]]) -- concordant minus discordant pairs off the
 * diagonal, the pairs not tied in i on it; tau-b is G_ij / sqrt(G_ii G_jj).  Exact, exactly symmetric, and the same bits on
 * every call.  GGL_E_ARG, found before any device work: an index outside [0,N) (the message names subset and position),
 * b < 2, B < 1, a rank outside [0,N), a shape beyond what one launch takes (p * b < 2^31, p <= 23104, ceil(b/64) * ceil(b/1024)
 * < 2^24: b up to about one million). */
int ggl_kendall_counts(int device, int p, int N, const int *ranks_host, int B, int b, const int *idx, long long *G_out);
/* S_out (B,p,p) = sin(pi/2 tau-b), diagonal exactly 1, exactly symmetric; G_out as above or NULL.  A variable that is constant
 * over a subset (G_ii = 0) is GGL_E_ARG naming subset and variable; nothing is written then. */
int ggl_kendall_skeptic(int device, int p, int N, const int *ranks_host, int B, int b, const int *idx, double *S_out,
                        long long *G_out);
/* ... straight into the S of a ctx whose K is a multiple of B: instance k gets the skeptic matrix of subset k % B, bitwise
 * that of the call above (layout and bookkeeping of ggl_set_S_from_subsets; the ctx keeps no variances).  GGL_E_ARG also for
 * a B that does not divide K and for a ctx with instance dimensions; a refused call leaves the ctx's S as it was. */
int ggl_set_S_from_kendall(ggl_ctx *ctx, const int *ranks_host, int N, int B, int b, const int *idx);

/* ---- Pairwise-complete covariance of data with missing values (covariance_missing.hip).  Entry points that are only ADDED:
 * GGL_VERSION stays where it is.
 *
 * A NaN entry of X is a missing value (+-Inf is a value, as in pandas; a pair that involves it is not finite).  For every pair
 * (i,j), the diagonal included, over the samples O_ij where both x_i and x_j are observed, n_ij = |O_ij|:
 *     S_ij = (1/n_ij) sum_{O_ij} (x_in - m_i|j)(x_jn - m_j|i),  m_i|j the mean of x_i over O_ij      (GGL_COV_CENTER)
 *     S_ij = (1/n_ij) sum_{O_ij} x_in x_jn                                                            (without)
 * -- R's cov(use = "pairwise.complete.obs") and pandas' DataFrame.cov() up to the factor (n_ij - 1) / n_ij.  S may be
 * indefinite; it is returned as it is.  Arguments, layouts and flags as ggl_covariance; counts_out (K,p,p) ints or NULL: n_ij.
 * S and the counts are exactly symmetric, two calls give the same bits, instance k's result does not depend on the others;
 * on data without NaN the counts all equal N[k].  GGL_COV_SCALE divides by the diagonal of THIS S, the variance of each
 * variable over all its observed entries, and returns it in scale_out: the diagonal becomes 1, but an off-diagonal entry,
 * whose covariance comes from other samples than the two variances, can exceed 1 in magnitude.
 * GGL_E_ARG, the message naming the offender: min_pairs < 1; a variable without any observed entry (instance, variable); a
 * pair with n_ij < min_pairs (instance, pair).  A refused call writes nothing to S_out, scale_out, counts_out. */
int ggl_covariance_pairwise(int device, int K, int p, const int *N, const double *const *X_host, int flags, int min_pairs,
                            double *S_out, double *scale_out, int *counts_out);
/* ... of B column subsets of ONE data array (arguments of ggl_covariance_subsets): subset r's matrix is bitwise what the call
 * above returns for the gathered (p,b) array in a call of K = B instances; the messages name the subset. */
int ggl_covariance_pairwise_subsets(int device, int p, int N, const double *X_host, int B, int b, const int *idx, int flags,
                                    int min_pairs, double *S_out, double *scale_out, int *counts_out);
/* ... straight into the S of a ctx (bookkeeping of ggl_set_S_from_subsets: the matrices are built beside the ctx's S and
 * installed once every check has passed).  Unlike ggl_set_S_from_data, a refused call leaves the ctx's S, its variances and
 * what was built for them as they were. */
int ggl_set_S_from_data_pairwise(ggl_ctx *ctx, const double *const *X_host, const int *N, int flags, int min_pairs);
int ggl_set_S_from_subsets_pairwise(ggl_ctx *ctx, const double *X_host, int N, int B, int b, const int *idx, int flags,
                                    int min_pairs);

/* ---- Weighted covariance of ONE data array under K weight rows (covariance_weighted.hip): the kernel-smoothed covariance
 * stack of a time series (Zhou, Lafferty, Wasserman 2010; Monti et al. 2014), observation weights, EM responsibilities.  Entry
 * points that are only ADDED: GGL_VERSION stays where it is.
 *
 * X_host the row-major (p,N) array, variables in rows; w_host the row-major (K,N) array of non-negative weights.  Per row k:
 *     W_k = sum_n w_kn,   m_k = (1/W_k) sum_n w_kn x_n,   S_k = (1/W_k) sum_n w_kn (x_n - m_k)(x_n - m_k)^T    (GGL_COV_CENTER)
 *     S_k = (1/W_k) sum_n w_kn x_n x_n^T                                                                        (without)
 * -- numpy.cov(X, aweights=w_k, bias=True).  X goes up once and is read by all K instances.  S_k is the Gram matrix of
 * sqrt(w_kn) (x_n - m_k): exactly symmetric and positive semidefinite up to rounding.  Instance k visits the samples between
 * the first and the last positive weight of its row only (from the multiple of 64 at or below the first), so the work follows
 * the support of the weights; on finite data the result is bitwise that of the loop over all N samples, which
 * GGL_COV_FULL_RANGE (tests, measurements) runs.  Fixed reduction orders: two calls give the same bits, and instance k's
 * result depends on X and row k alone.  A non-finite entry of X inside a support spreads over its row and column as in
 * ggl_covariance; outside every support its effect is unspecified (it is dropped by default and spreads with
 * GGL_COV_FULL_RANGE).
 * S_out (K,p,p); scale_out (K,p) or NULL (needed with GGL_COV_SCALE): the weighted variances; wsum_out (K) or NULL: the W_k the
 * kernels used.  flags as ggl_covariance, and GGL_COV_FULL_RANGE.
 * GGL_E_ARG, the message naming the offender: p, N or K < 1 (K <= 65535), a NULL buffer, an unknown flag bit, both TILE flags; a
 * negative or non-finite weight (instance, sample); a weight row whose sum is zero or not finite (instance); with GGL_COV_SCALE
 * a variable of zero or non-finite variance under that row's weights (instance, variable).  A refused call writes nothing to
 * S_out, scale_out, wsum_out. */
#define GGL_COV_FULL_RANGE 16 /* every instance loops over all N samples (tests, measurements) */
int ggl_covariance_weighted(int device, int p, int N, const double *X_host, int K, const double *w_host, int flags,
                            double *S_out, double *scale_out, double *wsum_out);
/* ... straight into the S of a ctx, K the ctx's (bookkeeping of ggl_set_S_from_subsets: the matrices are built beside the
 * ctx's S and installed once every check has passed; the variances are kept with GGL_COV_SCALE).  A refused call leaves the
 * ctx's S, its variances and what was built for them as they were. */
int ggl_set_S_from_weighted(ggl_ctx *ctx, const double *X_host, int N, const double *w_host, int flags);

/* ---- Latent correlation of mixed binary / continuous data: the Gaussian copula model of Fan, Liu, Ning, Zou (2017), the
 * estimator of R's mixedCCA / latentcor (bridge.hip behind the counts of kendall.hip).  Entry points that are only ADDED:
 * GGL_VERSION stays where it is.
 *
 * ranks_host, idx, B, b as ggl_kendall_counts.  types (p): 1 for a binary variable (its dense ranks are 0 and 1), 0 for a
 * continuous one.  Per subset, with n = b samples, tau = G_ij / (n (n - 1) / 2) (Kendall's tau-a of the exact counts G) and, for
 * a binary variable with n0 samples of rank 0, Delta = the standard normal quantile of n0 / n:
 *     continuous, continuous:  S_ij = sin(pi/2 tau)                                                         (not clipped)
 *     binary, binary:          S_ij = the root r of (1/pi) int_0^{asin r}        g(t; Delta_i, Delta_j) dt = tau
 *     binary, continuous:      S_ij = the root r of (2/pi) int_0^{asin(r/sqrt 2)} g(t; Delta, 0) dt         = tau
 *     g(t; h, k) = exp(-(h^2 + k^2 - 2 h k sin t) / (2 cos^2 t)),
 * sought in [-clip, clip]: tau at or beyond the bridge's value at an end gives that end, and such pairs are counted.  The
 * integral is a 64-node Gauss-Legendre rule, one node per lane of a wave; the root is a safeguarded Newton iteration.  Every
 * unordered pair is solved once and written twice: S is exactly symmetric, its diagonal exactly 1, two calls give the same
 * bits.  It need not be positive semidefinite.
 * S_out (B,p,p); G_out (B,p,p) the counts, n0_out (B,p) the samples of rank 0 of every variable, clipped_out (B) the clipped
 * pairs: each may be NULL.
 * GGL_E_ARG, the message naming the offender: what ggl_kendall_counts refuses; a types entry outside {0, 1}; a variable marked
 * binary with a rank above 1; a variable that is constant (over all samples: found on the host; over one subset: found on the
 * device, naming subset and variable); clip outside (0, 1).  A refused call writes nothing. */
int ggl_mixed_correlation(int device, int p, int N, const int *ranks_host, const int *types, int B, int b, const int *idx,
                          double clip, double *S_out, long long *G_out, int *n0_out, int *clipped_out);
/* ... straight into the S of a ctx whose K is a multiple of B (layout and bookkeeping of ggl_set_S_from_kendall), bitwise the
 * matrices of the call above.  A refused call leaves the ctx's S as it was. */
int ggl_set_S_from_mixed(ggl_ctx *ctx, const int *ranks_host, const int *types, int N, int B, int b, const int *idx,
                         double clip);

/* ---- Nearest-correlation projection of an indefinite S (nearcorr.hip around the L-step's (C - mu I)_+): Higham's (2002)
 * alternating projections with Dykstra's correction, what R's Matrix::nearPD does behind latentcor / mixedCCA.  The skeptic,
 * pairwise-complete and latent matrices above need not be positive semidefinite; this makes them so.  Entry points that are
 * only ADDED: GGL_VERSION stays where it is.
 *
 * A (B,p,p): symmetric matrices with a positive diagonal d (used as (A + A^T) / 2).  Per matrix, on D^-1/2 A D^-1/2 with the
 * diagonal set to exactly 1, starting from Y = A, dS = 0:
 *     R = Y - dS;   X = eps I + (R - eps I)_+;   dS = X - R;   Y' = X with the diagonal set to 1
 *     r1 = |Y' - Y|_F / |Y'|_F,   delta = |Y' - X|_F,   r2 = delta / |Y'|_F;   stop when max(r1, r2) <= tol
 * The B matrices run in lock-step; one that has stopped is frozen.  Then, always (also after max_iter iterations without
 * convergence): with nu = delta / (1 - eps + delta) the result is (1 - nu) Y' off the diagonal and 1 on it, scaled back by
 * sqrt(d_i d_j).  Since lambda_min(Y') >= eps - delta, its smallest eigenvalue is at least eps min_i d_i, and its diagonal is d.
 * A matrix that meets the stopping test in iteration 1 needed no projection and is returned bit for bit (iters = 1, nu = 0;
 * lambda_min >= eps - tol |A|_F then).  The result is exactly symmetric; two calls give the same bits.
 * iters (B): the iterations run, -max_iter where the tolerance was not reached (not an error: the shrunk iterate is feasible,
 * only not nearest).  info (B,4): max(r1, r2) of the last iteration, |out - A|_F, nu, eigendecomposition fallbacks of the
 * L-step over the call (the same number in every row).
 * GGL_E_ARG, the message naming the offender: B or p < 1, B > 65535, a NULL buffer, eps outside [0, 0.5], tol outside [1e-14, 1e-2],
 * max_iter < 1; a non-finite entry or a non-positive diagonal entry (instance, variable).  A refused call writes nothing. */
int ggl_nearest_correlation(int B, int p, const double *A, double *out, double eps, double tol, int max_iter, int *iters,
                            double *info);
/* ... of the S installed in a ctx, in place.  period = B > 0, a divisor of K: S holds B distinct matrices, instance k carrying
 * matrix k % B (the layout of ggl_set_S_ex and of the ggl_set_S_from_*subsets calls); the first B are projected and replicated
 * device to device.  period = 0 projects all K.  iters (B) and info (B,4) as above, B = K for period 0.  The variances kept
 * beside a correlation S stay as they are.  A refused call (also: a period that does not divide K) leaves S bit for bit. */
int ggl_project_S(ggl_ctx *ctx, int period, double eps, double tol, int max_iter, int *iters, double *info);

/* ---- Debiased (de-sparsified) graphical lasso: the statistics behind edge-wise tests and confidence intervals (Jankova,
 * van de Geer 2015; D-S_GL of R's SILGGM) on the FP64 matrix cores (debias.hip).  An entry point that is only ADDED:
 * GGL_VERSION stays where it is.
 *
 * Theta_host (K,p,p): the estimates, symmetric; S_host (K,p,p): the covariances they were fitted to, symmetric; n (K) doubles:
 * the (effective, not necessarily integer) numbers of observations.  Per instance
 *     T  = 2 Theta - Theta S Theta                                (the debiased estimate; not sparse)
 *     SE = sqrt((Theta_ii Theta_jj + Theta_ij^2) / n_k)           (the asymptotic standard error of T_ij)
 * so that (T_ij - Theta0_ij) / SE_ij is asymptotically N(0,1).  Two launches: M = Theta S as a full product, then M Theta
 * over the tile pairs I <= J with both epilogues fused; Theta_ij, Theta_ii, Theta_jj are read from the upper triangle.
 * T_out, SE_out (K,p,p).  Every pair is evaluated once and written twice: both stacks are bitwise symmetric.  Fixed
 * reduction order, no atomics: two calls give the same bits, and instance k's result does not depend on K or on the other
 * instances.  Any p >= 1.
 * flags: 0, or one of the forced tile shapes below (tests, measurements); the default is 64 x 64 where K T (T + 1) / 2
 * tile pairs fill the chip, else 32 x 32.
 * GGL_E_ARG, found on the host before any device work, the message naming the offender: K or p < 1, a NULL buffer, any other
 * flag bit or both tile flags; a non-finite entry of Theta or S (instance, row, column); Theta_ii <= 0 (instance, variable);
 * n_k <= 0 or not finite (instance).  A refused call writes nothing to T_out, SE_out. */
#define GGL_DEBIAS_TILE32 4
#define GGL_DEBIAS_TILE64 8
int ggl_debias(int device, int K, int p, const double *Theta_host, const double *S_host, const double *n, int flags,
               double *T_out, double *SE_out);
/* measurement: average milliseconds of `iters` launches on random device data (HIP events); ms_out[0] the full product
 * M = A T (launch_gemm_right), ms_out[1] k_debias with its epilogues.  tile: 0 (by size), 32, 64. */
int ggl_dev_debias_bench(int K, int p, int tile, int iters, double *ms_out);

/* ---- Gaussian predictive scores by a batched FP64 Cholesky factorisation (cholesky.hip): the log det and the
 * quadratic form behind the leave-one-out choice of a kernel bandwidth (Yin et al. 2010; Monti et al. 2014).  Entry points
 * that are only ADDED: GGL_VERSION stays where it is.
 *
 * ggl_cholesky_predict: S_host (K,p,p) symmetric (only the lower triangle is read), d_host (K,p) or NULL, ridge >= 0 added
 * to every diagonal.  out (K,4) per instance:
 *     out[0] = log det (S + ridge I) = 2 sum_j log l_jj        out[1] = d^T (S + ridge I)^-1 d   (0 with d_host NULL)
 *     out[2] = the smallest pivot l_jj^2                        out[3] = status
 * status is -1 if every pivot a_jj - sum_m l_jm^2 was positive and finite, else the first column whose pivot was not; then
 * out[0] = -inf, out[1] = NaN and out[2] is the smallest pivot up to and including the failing one (NaN if that one is NaN).
 * A matrix that is not positive definite, or holds a NaN, is a status and not an error.  One workgroup per matrix, any
 * p >= 1, fixed summation orders and no atomics: two calls give the same bits and instance k's bits do not depend on K.
 * GGL_E_ARG before any device work, nothing written to out: K or p < 1, S_host or out NULL, ridge negative or not finite.
 *
 * ggl_weighted_predictive_scores: row r of w_host (M,N) weights the columns of X_host (p,N) as in ggl_covariance_weighted
 * (same kernels, S_r bit for bit); the call scores column target[r] of X under the Gaussian with that mean and covariance:
 * d = x_target - m_r, formed on the device from the weighted means (without GGL_COV_CENTER: d = x_target, S_r the weighted
 * raw second moment), out (M,4) as above for (S_r, d).  w[r,target[r]] need not be 0; a leave-one-out caller sets it.
 * X goes up once; the rows are processed `chunk` at a time, chunk = 0 sizing the chunk so that its covariance stack takes
 * at most 256 MiB (and at most 65535 rows).  out does not depend on chunk, bit for bit.
 * flags: 0 or GGL_COV_CENTER, | GGL_COV_FULL_RANGE, | one of GGL_COV_TILE32 / GGL_COV_TILE64.
 * GGL_E_ARG before any device work, nothing written to out: what ggl_covariance_weighted refuses, with its messages (also a
 * negative or non-finite weight and a weight row without a positive weight, found on the host here); GGL_COV_SCALE; ridge
 * negative or not finite; a target outside [0,N) (the row is named); chunk < 0; a NULL buffer; M or p < 1. */
int ggl_cholesky_predict(int device, int K, int p, const double *S_host, const double *d_host, double ridge, double *out);
int ggl_weighted_predictive_scores(int device, int p, int N, const double *X_host, int M, const double *w_host,
                                   const int *target, double ridge, int flags, int chunk, double *out);
/* measurement: average milliseconds of `iters` launches of k_chol_predict on K random SPD (p,p) matrices with right-hand
 * sides (HIP events, the stack restored by a device copy in front of every launch; ms_out[2] is that copy alone):
 * ms_out[0] the update on the matrix cores, ms_out[1] the same kernel with the update on the VALU. */
int ggl_dev_chol_bench(int K, int p, int iters, double *ms_out);

/* ---- Meinshausen-Buhlmann neighbourhood selection (2006; method = "mb" of R's huge): one lasso per node on a shared matrix
 * (neighborhood.hip).  Entry points that are only ADDED: GGL_VERSION stays where it is.
 *
 * For a symmetric S with positive diagonal, node j and lambda > 0:
 *     beta^(j) = argmin over beta with beta_j = 0 of  1/2 beta' S beta - s_j' beta + lambda sum_{k != j} |beta_k|
 * by cyclic coordinate descent with covariance updates on an active set, one wave per (matrix, node), the grid walked in
 * descending order inside the kernel with warm starts.  A (node, lambda) is finished only in a state where the gradient
 * recomputed from beta, one further sweep and one further screen of all variables move nothing beyond tol and find no
 * violator.  Largest p: 2048.
 *
 * ggl_neighborhood_path: S_host (M,p,p); lam (L) strictly descending, positive, finite; tol bounds a sweep's
 * max_k |change of beta_k| S_kk; max_sweeps caps the sweeps of one (node, lambda).
 *   coef_out (M,L,p,p):  rule GGL_MB_RAW: column j holds beta^(j).  GGL_MB_AND / GGL_MB_OR: for i < j, of a = beta^(j)_i and
 *                        b = beta^(i)_j the one of smaller / larger magnitude, a on a tie, written to (i,j) and (j,i):
 *                        bitwise symmetric with a zero diagonal
 *   resvar_out (M,L,p) or NULL:  tau_j^2 = S_jj - 2 s_j' beta + beta' S beta
 *   info_out (M,L,p,2) int32:  sweeps, status -- 0 converged, 1 a cap was reached (max_sweeps, or 100 screens), 2 a
 *                        non-finite value: beta^(j) is NaN at this lambda and every later one
 * No atomics, fixed summation orders: two calls give the same bits, matrix m's do not depend on M, and lambda l's do not
 * depend on the lambdas behind it.
 * GGL_E_ARG before any device work, nothing written: M, L or p < 1; p > 2048; a NULL buffer other than resvar_out; a lambda
 * that is not positive and finite (named); a grid that is not strictly descending; tol negative or not finite;
 * max_sweeps < 1; an unknown rule; a non-finite entry or a non-positive diagonal entry of S_host (matrix and index named).
 *
 * ggl_neighborhood_stability: the same path on the S of a ctx, its K instances taken as B = K matrices (what
 * ggl_set_S_from_subsets, _kendall, _mixed, _pairwise and ggl_project_S leave there: the data went up once, the matrices never
 * exist on the host), rule GGL_MB_AND or GGL_MB_OR.  The symmetrised (L,B,p,p) stack stays on the device and is reduced by the
 * kernel of ggl_edge_stability: num_out (L) and counts_out (L,p,p) int32 or NULL as there, for |W_ij| >= t.  stack_out
 * (L,B,p,p) or NULL; info_out (L,B,p,2) as above.  S is on the device: a non-finite value there is status 2 of the nodes it
 * reaches, not an error.  GGL_E_ARG as above (without the checks of S_host), also: GGL_MB_RAW, t negative or not finite, a ctx
 * with instance dimensions. */
#define GGL_MB_RAW 0
#define GGL_MB_AND 1
#define GGL_MB_OR 2
int ggl_neighborhood_path(int device, int M, int p, const double *S_host, int L, const double *lam, int rule, double tol,
                          int max_sweeps, double *coef_out, double *resvar_out, int *info_out);
int ggl_neighborhood_stability(ggl_ctx *ctx, int L, const double *lam, int rule, double tol, int max_sweeps, double t,
                               long long *num_out, int *counts_out, double *stack_out, int *info_out);

/* ---- Refit of neighbourhood selection on its graph (mb_refit.hip): with the graph held fixed every node is
 * regressed on its neighbours by ordinary least squares.  This is the relaxed lasso (Meinshausen 2007, Comput. Statist. Data
 * Anal. 52) and the regression-based precision estimator of Yuan (2010, JMLR 11) and Zhou, Ruetimann, Xu, Buehlmann (2011,
 * JMLR 12); held-out prediction error of the regressions is how the 2006 paper tunes lambda.  Entry points that are only
 * ADDED: GGL_VERSION stays where it is.
 *
 * Per (matrix m, graph g, node j), with W_host (M,G,p,p) and S_host (M,p,p):
 *     A      = { i != j : |W[m,g,j,i]| >= t }     ROW j, ascending; a NaN is no edge; W need not be symmetric
 *     beta   = S_AA^-1 s_A,  s_A = S[A, j]         Cholesky
 *     tau^2  = q(S; beta),  r = q(T; beta),        q(M; b) = M_jj - 2 m_A' b + b' M_AA b
 *   coef_out (M,G,p,p):  column j holds beta^(j), zero off A
 *   resvar_out (M,G,p);  heldout_out (M,G,p) or NULL: r, needs T_host (M,p,p)
 *   info_out (M,G,p,2):  the degree |A| and a status: 0 solved / 1 a pivot was not positive and finite (S_AA is not positive
 *                        definite) / 2 a non-finite value among the gathered entries (of T here: S_host is checked) / 3 the
 *                        degree exceeds the cap.  For 1, 2, 3 that node's tau^2, r and column of coef are NaN (diagonal 0);
 *                        nobody else is touched and nothing is an error.
 * ggl_mb_refit_limits: out[0] the degree cap (128), out[1] the largest p (2048).
 * Reproducible: fixed summation orders, no atomics; the bits of (m,g) depend neither on M nor on G.
 * GGL_E_ARG before any device work, nothing written: M, G or p < 1; p > 2048; a NULL S_host, W_host, coef_out, resvar_out or
 * info_out; heldout_out without T_host; t negative or not finite; a non-finite entry or a non-positive diagonal entry of
 * S_host (matrix and index named).
 *
 * ggl_neighborhood_cv: one whole cross-validation step on a ctx whose K = F instances hold the train matrices of the folds
 * (ggl_set_S_from_subsets and its siblings, ggl_project_S).  The path runs and is symmetrised as in
 * ggl_neighborhood_stability (rule GGL_MB_AND or GGL_MB_OR); the F test covariances are built from X_host (p,N) and idx_test
 * (F,m) exactly as ggl_heldout_scores builds them (flags: GGL_COV_CENTER or 0); then, refit != 0: the refit above with
 * S = train, T = test, W = the symmetrised stack; refit == 0: the lasso's own beta and tau^2, and r = q(T; beta).
 *   resvar_out, heldout_out (L,F,p);  info_out (L,F,p,2): (degree, status) of the refit, or with refit == 0 (sweeps, status)
 *   of the path;  stack_out (L,F,p,p) or NULL: the symmetrised stack.  The matrices never exist on the host.
 * GGL_E_ARG: what ggl_neighborhood_stability and ggl_heldout_scores refuse; a ctx with K != F. */
void ggl_mb_refit_limits(int out[2]);
int ggl_neighborhood_refit(int device, int M, int p, const double *S_host, int G, const double *W_host, double t,
                           const double *T_host, double *coef_out, double *resvar_out, double *heldout_out, int *info_out);
int ggl_neighborhood_cv(ggl_ctx *ctx, const double *X_host, int N, int F, int m, const int *idx_test, int flags, int L,
                        const double *lam, int rule, double tol, int max_sweeps, double t, int refit, double *resvar_out,
                        double *heldout_out, int *info_out, double *stack_out);

/* ---- Neighbourhood selection with per-entry penalty weights and the scaled lasso (neighborhood.hip).
 * Weights: the adaptive lasso (Zou 2006, JASA 101), glmnet's penalty.factor.  Scaled lasso: Sun & Zhang (2012, Biometrika 99;
 * precision matrix: 2013, JMLR 14, R's scalreg), the square-root lasso of Belloni, Chernozhukov, Wang (2011, Biometrika 98),
 * the estimator behind TIGER (Liu & Wang 2017, EJS 11; method = "tiger" of R's huge / flare).  Entry points that are only
 * ADDED: GGL_VERSION stays where it is.
 *
 * Node j has the weights w_k = weights[j,k] in [0, +inf] (ROW j; the diagonal is not read) and, with g = s_j - S beta and
 * tau^2(beta) = S_jj - 2 s_j' beta + beta' S beta:
 *     GGL_MB_LASSO:   min 1/2 beta' S beta - s_j' beta + lambda sum_k w_k |beta_k|      thr_k = lambda w_k
 *     GGL_MB_SCALED:  min sqrt(tau^2(beta)) + lambda sum_k w_k |beta_k|                  thr_k = lambda sigma w_k, sigma = tau
 * w_k = 0: an unpenalised coordinate; w_k = +inf: an excluded one, its coefficient is exactly 0.  GGL_MB_LASSO is the
 * procedure of ggl_neighborhood_path with thr_k in place of lambda; with unit weights it returns that entry's bits.
 * GGL_MB_SCALED alternates, per (node, lambda): sigma_t = sqrt(tau^2) of the warm start (sqrt(S_jj) at the first lambda) ->
 * that procedure at lambda sigma_t w_k -> sigma_new = sqrt(tau^2) -> finished if |sigma_new - sigma_t| <= sig_tol sigma_new,
 * else again with sigma_new, at most max_outer times.  resvar is the final tau^2: in scaled mode sigma_j^2.
 *
 * Each entry is its sibling (ggl_neighborhood_path, _stability, _cv) plus
 *   weights (p,p), with weights_per_matrix != 0 (M,p,p) / (K,p,p) / (F,p,p): host memory; NULL: all 1
 *   mode, sig_tol, max_outer (the last two are checked in both modes and used in GGL_MB_SCALED)
 * and its info holds THREE ints per (matrix, lambda, node): sweeps, status, outer iterations (0 with GGL_MB_LASSO).  Status
 * 0 finished / 1 a cap was reached (max_sweeps, 100 screens, max_outer) / 2 a non-finite value / 3 GGL_MB_SCALED only:
 * tau^2 <= 1e-10 S_jj or not positive, the square-root problem is degenerate (a duplicated variable, a perfect fit).  For 2
 * and 3 the node is NaN (diagonal 0) at this lambda and every later one.  ggl_neighborhood_cv_w with refit != 0 returns the
 * refit's info, two ints per node as its sibling does, in the leading part of info_out; info_out has room for three.
 * GGL_E_ARG before any device work, nothing written: what the sibling refuses; a weight that is negative or NaN (matrix, row
 * and column named; +inf is legal); an unknown mode; sig_tol negative or not finite; max_outer < 1. */
#define GGL_MB_LASSO 0
#define GGL_MB_SCALED 1
int ggl_neighborhood_path_w(int device, int M, int p, const double *S_host, int L, const double *lam, int rule, double tol,
                            int max_sweeps, const double *weights, int weights_per_matrix, int mode, double sig_tol,
                            int max_outer, double *coef_out, double *resvar_out, int *info_out);
int ggl_neighborhood_stability_w(ggl_ctx *ctx, int L, const double *lam, int rule, double tol, int max_sweeps, double t,
                                 const double *weights, int weights_per_matrix, int mode, double sig_tol, int max_outer,
                                 long long *num_out, int *counts_out, double *stack_out, int *info_out);
int ggl_neighborhood_cv_w(ggl_ctx *ctx, const double *X_host, int N, int F, int m, const int *idx_test, int flags, int L,
                          const double *lam, int rule, double tol, int max_sweeps, double t, int refit, const double *weights,
                          int weights_per_matrix, int mode, double sig_tol, int max_outer, double *resvar_out,
                          double *heldout_out, int *info_out, double *stack_out);

/* ---- Joint neighbourhood selection of K instances under the GGL penalty (neighborhood_joint.hip).  Entry points
 * that are only ADDED: GGL_VERSION stays where it is.
 *
 * The regression counterpart of reg = 'GGL' (Chiquet, Grandvalet, Ambroise 2011; Danaher, Wang, Witten 2014): for node j
 *     min_B  sum_k omega_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ]
 *            + lam1 sum_k sum_{i != j} |beta^(k)_i| + lam2 sum_{i != j} ||(beta^(1)_i, ..., beta^(K)_i)||_2 ,   beta^(k)_j = 0,
 * by block coordinate descent on an active set of groups (one block: the K coefficients of one variable; its solution is the
 * root of a scalar equation, found by a monotone Newton iteration), with the screen / sweep / recompute / confirm procedure,
 * the caps and the statuses of ggl_neighborhood_path.
 *
 * ggl_neighborhood_joint_path: S_host (K,p,p), every S[k] bitwise symmetric, finite, with a positive diagonal; omega (K)
 * positive and finite, or NULL (all 1); lam1, lam2 (C,L): C chains of L penalty pairs, each chain walked in order with warm
 * starts (no order is asked of the pairs); lam1, lam2 >= 0, finite, lam1 + lam2 > 0.  rule is applied per instance to every
 * (c,l,k) matrix as in ggl_neighborhood_path.
 *   coef_out (C,L,K,p,p) or NULL;  resvar_out (C,L,K,p) or NULL: S^(k)_jj - 2 s_j^(k)' beta^(k) + beta^(k)' S^(k) beta^(k), unweighted
 *   info_out (C,L,p,3): sweeps, status (0 finished / 1 a cap was reached: max_sweeps, 100 screens / 2 a non-finite value: all K
 *     columns of that node are NaN, diagonal 0, at this pair and every later one of the chain, nobody else is touched), the
 *     largest number of Newton steps one block took
 *   refit != 0 (rule GGL_MB_AND or GGL_MB_OR): every (c,l,k) matrix is refitted on its graph (|W| >= t) against S[k] by the
 *     kernels of ggl_neighborhood_refit, on the device; refit_coef_out (C,L,K,p,p), refit_resvar_out (C,L,K,p),
 *     refit_info_out (C,L,K,p,2: degree, status as there), each or NULL.
 * The same bits on every call; a chain's do not depend on C or on the other chains, a pair's not on the pairs behind it.
 * The device stack is processed in chunks of chains under a fixed memory budget; the outputs do not depend on the chunking
 * (ggl_mb_joint_chunk_budget sets the budget in bytes for tests, 0 restores the default).
 * ggl_neighborhood_joint_last: the same call, but coef_out and refit_coef_out are (C,K,p,p) and receive the LAST pair of every
 * chain only (the tables stay whole): what a search wants of the chain that leads to its chosen point.
 * ggl_mb_joint_limits: out[0] = largest K (64), out[1] = largest p (1024); every (K, p) inside is served.  The K gradients of a
 * node live in the registers of one workgroup where they fit (K <= 64 up to p = 384, 32 up to 512, 16 up to 1024) and in a
 * workspace in device memory beyond: the same procedure, slower.
 * ggl_dev_mb_joint_bench: the path kernel alone on all C chains, HIP-event times of iters launches in ms_out (for tools).
 * GGL_E_ARG before any device work, nothing written, the message naming the offender: K, p, C or L < 1 or beyond the limits; a
 * NULL S_host, lam1, lam2 or info_out; a penalty that is negative or not finite, or a pair with lam1 + lam2 = 0 (chain, index);
 * an omega that is not positive and finite; tol negative or not finite; max_sweeps < 1; an unknown rule; GGL_MB_RAW with
 * refit; with refit, t negative or not finite; an entry of S_host that is not finite or a diagonal entry that is not positive
 * (instance, index); an S_host[k] that is not bitwise symmetric (instance, pair). */
void ggl_mb_joint_limits(int out[2]);
void ggl_mb_joint_chunk_budget(long long bytes);
int ggl_neighborhood_joint_last(int device, int K, int p, const double *S_host, const double *omega, int C, int L,
                                const double *lam1, const double *lam2, int rule, double tol, int max_sweeps, int refit, double t,
                                double *coef_out, double *resvar_out, int *info_out, double *refit_coef_out,
                                double *refit_resvar_out, int *refit_info_out);
int ggl_dev_mb_joint_bench(int K, int p, const double *S_host, int C, int L, const double *lam1, const double *lam2, double tol,
                           int max_sweeps, int iters, double *ms_out);
int ggl_neighborhood_joint_path(int device, int K, int p, const double *S_host, const double *omega, int C, int L,
                                const double *lam1, const double *lam2, int rule, double tol, int max_sweeps, int refit, double t,
                                double *coef_out, double *resvar_out, int *info_out, double *refit_coef_out,
                                double *refit_resvar_out, int *refit_info_out);

/* ---- Fused joint neighbourhood selection of K ORDERED instances (neighborhood_fused.hip).  Entry points that are
 * only ADDED: GGL_VERSION stays where it is.
 *
 * The regression counterpart of reg = 'FGL' (time-varying neighbourhood selection: Kolar, Song, Ahmed, Xing 2010; the penalty
 * of Danaher, Wang, Witten 2014): for node j, in the instances' given order,
 *     min_B  sum_k omega_k [ 1/2 beta^(k)' S^(k) beta^(k) - s_j^(k)' beta^(k) ]
 *            + lam1 sum_k sum_{i != j} |beta^(k)_i| + lam2 sum_{i != j} sum_{k < K} |beta^(k+1)_i - beta^(k)_i| ,   beta^(k)_j = 0,
 * by block coordinate descent (one block: the K coefficients of one variable, updated by the fused-lasso prox under the one
 * curvature max_k omega_k S^(k)_ii -- exact where these are equal, a majorise-minimise step with the same fixed points
 * otherwise; the total-variation prox is Condat's direct scan).
 *
 * ggl_neighborhood_fused_path, ggl_neighborhood_fused_last: the arguments, the outputs, the statuses, the chunking (and its
 * budget, ggl_mb_joint_chunk_budget) and the GGL_E_ARG refusals of ggl_neighborhood_joint_path / _last; the third info column
 * is 0.  lam2 > 0 with K = 1 is accepted and inert.
 * ggl_mb_fused_limits: out[0] = largest K (64), out[1] = largest p (1024); every (K, p) inside is served (gradients in
 * registers for K <= 64 up to p = 384, 32 up to 512, 8 up to 1024; in a device workspace beyond).
 * ggl_dev_mb_fused_bench: as ggl_dev_mb_joint_bench, for k_mb_fused_path. */
void ggl_mb_fused_limits(int out[2]);
int ggl_neighborhood_fused_last(int device, int K, int p, const double *S_host, const double *omega, int C, int L,
                                const double *lam1, const double *lam2, int rule, double tol, int max_sweeps, int refit, double t,
                                double *coef_out, double *resvar_out, int *info_out, double *refit_coef_out,
                                double *refit_resvar_out, int *refit_info_out);
int ggl_dev_mb_fused_bench(int K, int p, const double *S_host, int C, int L, const double *lam1, const double *lam2, double tol,
                           int max_sweeps, int iters, double *ms_out);
int ggl_neighborhood_fused_path(int device, int K, int p, const double *S_host, const double *omega, int C, int L,
                                const double *lam1, const double *lam2, int rule, double tol, int max_sweeps, int refit, double t,
                                double *coef_out, double *resvar_out, int *info_out, double *refit_coef_out,
                                double *refit_resvar_out, int *refit_info_out);

#ifdef __cplusplus
}
#endif
#endif
