/*
 * limo_hip.h — C-ABI of the MI355X-native LIMO hot path (keyframe bundle adjustment + LiDAR depth assignment).
 *
 * This header is the drop-in boundary.  Everything above it (window bookkeeping, landmark/keyframe
 * selection, ROS I/O) stays in the host language; everything below it runs as hand-written HIP kernels
 * on gfx950.  Plain pointers and sizes only; no C++ types, no torch types, nothing thrown across it.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference tree):
 *
 *   limo_ba_solve / limo_ba_batch_*     the body of BundleAdjusterKeyframes::solve() between "selection
 *                                       done" and "return report":
 *                                       keyframe_bundle_adjustment/src/bundle_adjuster_keyframes.cpp:695-766
 *                                       (problem build :498-627, :769-818, :890-904; constness :198-219,
 *                                       :722-736; trimming schedule :740-758; solveTrimmed call :765) and
 *                                       robust_optimization/src/robust_solving.cpp:140-248 + ceres::Solve
 *                                       (Ceres 1.13, DENSE_SCHUR, Levenberg-Marquardt).
 *   limo_ba_adjust_pose_only            BundleAdjusterKeyframes::adjustPoseOnly(),
 *                                       bundle_adjuster_keyframes.cpp:820-888.
 *   limo_ba_adjust_pose_only_batch /    the same call for N independent frames at once (several sequences replayed side by
 *   limo_ba_batch_create_pose_only      side, many frames relocalised against a map): one pack, one upload, one launch.
 *   limo_ba_evaluate                    ceres::Problem::Evaluate as used at
 *                                       robust_optimization/src/robust_solving.cpp:44 and
 *                                       keyframe_bundle_adjustment/src/definitions.cpp:94 (residuals, cost) plus
 *                                       the Jacobians Ceres builds inside Solve for the blocks created at
 *                                       bundle_adjuster_keyframes.cpp:584-620
 *                                       (internal/cost_functors_ceres.hpp:53-222).
 *   limo_landmark_init                  BundleAdjusterKeyframes::calculateLandmark (both overloads),
 *                                       bundle_adjuster_keyframes.cpp:332-382, internal/triangulator.hpp:51-75.
 *   limo_trim_quantile                  TrimmerQuantile::getOutliers,
 *                                       robust_optimization/include/robust_optimization/internal/trimmer_quantile.hpp:40-63.
 *   limo_depth_estimate                 the (un-vendored) mono_lidar_depth DepthEstimator as pinned by
 *                                       demo_keyframe_bundle_adjustment_meta/res/mono_lidar_fusion_parameters.yaml:1-185;
 *                                       contract = FeaturePoint::d, matches_msg_types/include/matches_msg_types/feature_point.hpp:24-26.
 *
 * Conventions (reference: internal/definitions.hpp:23,75-83, keyframe.hpp:181-182):
 *   pose   = (qw,qx,qy,qz,tx,ty,tz), x' = R(q) x + t, keyframe <- origin.  Camera extrinsic = camera <- vehicle.
 *   All parameters are double; measurements are float and are widened exactly as the reference does
 *   (bundle_adjuster_keyframes.cpp:585,606-607).  A measurement without depth carries d < 0 (the solve
 *   uses d > 0.0f, :578).
 *
 * Return codes: 0 = ok, < 0 = invalid input / runtime error (see limo_last_error), > 0 reserved.
 * Threading: one limo_ctx per (thread, GPU, stream); calls on one ctx are serialised by the caller.
 */
#ifndef LIMO_HIP_H_
#define LIMO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIMO_ABI_VERSION 6 /* (still 6 with limo_ba_batch_solve_each / limo_ba_adjust_pose_only_batch_each, with limo_ba_batch_create_pose_only / limo_ba_adjust_pose_only_batch, with limo_ctx_last_solve_info and with limo_ba_solve_fixed_landmarks / limo_ba_batch_create_fixed_landmarks: more symbols, no layout changes) 6: limo_depth_params carries the whole parameter file, LIMO_ERR_UNSUPPORTED, limo_depth_last_reasons; 5: limo_ctx_comm_init_host; 2: limo_ba_evaluate_rows, limo_ctx_exchange_stats, limo_depth_last_ground_plane, limo_depth_set_timing, limo_depth_last_kernel_ms; 3: limo_ctx_coop_fallbacks; 4: limo_depth_estimate_begin / _end */

/* Keyframe::FixationStatus, keyframe.hpp:30 */
enum limo_fixation { LIMO_FIX_POSE = 0, LIMO_FIX_SCALE = 1, LIMO_FIX_NONE = 2 };

/* error codes */
enum limo_status {
    LIMO_OK = 0,
    LIMO_ERR_INVALID = -1,      /* null pointer, negative size, index out of range        */
    LIMO_ERR_NOT_ENOUGH_KF = -2, /* solve() on a window without active keyframes.  The reference's
                                    NotEnoughKeyframesException counts all PUSHED keyframes (< 3,
                                    bundle_adjuster_keyframes.cpp:630): the caller's check; the window of
                                    ACTIVE keyframes may hold 1 or 2 and is solved like the reference does */
    LIMO_ERR_RUNTIME = -3,      /* HIP runtime error                                       */
    LIMO_ERR_NO_DEVICE = -4,    /* no gfx950 device / extension cannot run                 */
    LIMO_ERR_UNSUPPORTED = -5   /* a setting the parameter file defines but this library does not build
                                   (limo_last_error names the key)                          */
};

/* Termination of one Ceres-style solve (ceres::TerminationType restated). */
enum limo_termination { LIMO_CONVERGENCE = 0, LIMO_NO_CONVERGENCE = 1, LIMO_FAILURE = 2 };

/*
 * One optimisation window, flattened (struct of arrays).  The caller owns every buffer; the library keeps
 * no pointer after a call returns.  Arrays marked inout are optimised in place, exactly like Ceres does
 * through the raw pointers the reference hands it (bundle_adjuster_keyframes.cpp:592-593,555-556).
 *
 * Keyframes are the ACTIVE keyframes in ascending keyframe-id (timestamp) order — the order of
 * active_keyframe_ids_ (std::set) that the regularisers iterate (:775,:892).
 * Landmarks are the SELECTED landmarks that exist in landmarks_, ascending landmark id.
 * Observations: one per (keyframe, landmark, camera) measurement of a selected landmark in an active
 * keyframe (:569-576); any order.
 */
typedef struct limo_ba_window {
    int32_t n_kf;
    int32_t n_cam;
    int32_t n_lm;
    int32_t n_obs;

    double* kf_pose;            /* [n_kf*7] inout                                         */
    double* kf_plane_dir;       /* [n_kf*3] inout  Plane::direction                        */
    double* kf_plane_dist;      /* [n_kf]   inout  Plane::distance (< -10: no ground plane) */
    const int32_t* kf_fixation; /* [n_kf] enum limo_fixation                               */

    const double* cam;          /* [n_cam*10] f, cx, cy, qw,qx,qy,qz, tx,ty,tz (camera<-vehicle) */

    double* lm_pos;             /* [n_lm*3] inout                                          */
    const double* lm_weight;    /* [n_lm]  Landmark::weight                                */
    const uint8_t* lm_is_ground;/* [n_lm]  Landmark::is_ground_plane                       */

    const int32_t* obs_kf;      /* [n_obs] index into keyframes of this window             */
    const int32_t* obs_lm;      /* [n_obs] index into landmarks of this window             */
    const int32_t* obs_cam;     /* [n_obs] index into cameras of this window               */
    const float* obs_u;         /* [n_obs]                                                 */
    const float* obs_v;         /* [n_obs]                                                 */
    const float* obs_d;         /* [n_obs] depth along camera z, < 0 = none                */
} limo_ba_window;

/*
 * Options.  Defaults (limo_ba_default_options) are the reference's: OutlierRejectionOptions
 * (bundle_adjuster_keyframes.hpp:79-89), robust_optimization::getStandardSolverOptions
 * (robust_solving.hpp:93-108), bundle_adjuster_keyframes.cpp:740-764, and Ceres 1.13 Solver::Options defaults.
 */
typedef struct limo_ba_options {
    double depth_thres;            /* 0.16  Cauchy scale, depth blocks        */
    double reprojection_thres;     /* 1.6   Cauchy scale, reprojection blocks */
    double depth_quantile;         /* 0.95                                    */
    double reprojection_quantile;  /* 0.95                                    */
    int32_t num_trim_rounds;       /* 1   outlier_rejection_options_.num_iterations */
    int32_t trim_solver_iterations;/* 2   entries of number_iterations        */
    int32_t min_landmarks_for_trimming; /* 100: trimming only if n_lm > this (solve); 30 for pose-only */
    int32_t minimum_number_residual_groups; /* 30 */
    int32_t max_num_iterations;    /* 100 */
    double max_solver_time_sec;    /* wall-clock cap per ceres-style solve; <= 0 disables it (deterministic). */
    /* Ceres 1.13 trust-region defaults */
    double function_tolerance;     /* 1e-6  */
    double gradient_tolerance;     /* 1e-10 */
    double parameter_tolerance;    /* 1e-8  */
    double initial_trust_region_radius; /* 1e4  */
    double max_trust_region_radius;     /* 1e16 */
    double min_trust_region_radius;     /* 1e-32 */
    double min_lm_diagonal;        /* 1e-6  */
    double max_lm_diagonal;        /* 1e32  */
    double min_relative_decrease;  /* 1e-3  */
    int32_t max_num_consecutive_invalid_steps; /* 5 */
    int32_t jacobi_scaling;        /* 1 */
} limo_ba_options;

/* What the reference returns as a FullReport() string, as numbers. */
typedef struct limo_ba_report {
    int32_t termination;         /* enum limo_termination of the FINAL solve                    */
    int32_t num_solves;          /* ceres-style solves executed (trim rounds [+retries] + final) */
    int32_t iterations_total;    /* LM iterations over all solves (iteration 0 not counted).  An iteration that ENDS its solve
                                    inside the step decision - parameter tolerance, function tolerance, the last of
                                    max_num_consecutive_invalid_steps invalid steps - IS counted here; Ceres' own count and the
                                    iteration log (limo_ba_iteration below) have no entry for it: at most one per solve */
    int32_t iterations_final;    /* LM iterations of the final solve                             */
    int32_t successful_steps;    /* accepted steps over all solves                               */
    int32_t n_depth_blocks;      /* residual blocks built (before trimming)                      */
    int32_t n_repr_blocks;
    int32_t n_gp_blocks;
    int32_t n_trimmed_landmarks; /* landmarks removed by trimming                                */
    int32_t num_linearizations;  /* residual+Jacobian evaluations (iteration 0 + accepted steps), all solves */
    double initial_cost;         /* cost of the first solve at x0 (incl. fixed cost)             */
    double final_cost;           /* cost after the final solve (incl. fixed cost)                */
    double time_sec;             /* wall time inside the library for this window / batch         */
} limo_ba_report;

typedef struct limo_ctx limo_ctx;
typedef struct limo_ba_batch limo_ba_batch;

/* --- context ------------------------------------------------------------------------------------ */
int limo_abi_version(void);
/* A context = one GPU + one stream + the scratch it reuses between calls.  Not thread-safe: one context per host
 * thread (several contexts may share a GPU).  Device blocks and pinned staging buffers released by finished calls stay with
 * the context for the next call and are freed by limo_ctx_destroy: up to 32 MB a few per power-of-two size class, larger ones
 * (the arena of a big batch) one per 64 MB class and at most 16 GB altogether.  Idle blocks never cost an allocation: when the
 * device is out of memory they are released, largest first, and the allocation is tried again.  HOST side: a context that has
 * created a batch of 128 windows or more keeps ONE page-locked arena (sized for that batch, at most 1 GB) that the flattened
 * arrays of its next large batches are written into and uploaded from - one live batch at a time holds it, the others use the
 * heap. */
int limo_ctx_create(int device, limo_ctx** out);
void limo_ctx_destroy(limo_ctx* ctx);
/* Use an existing hipStream_t (e.g. the host framework's current stream); NULL = the context's own. */
int limo_ctx_set_stream(limo_ctx* ctx, void* hip_stream);
const char* limo_last_error(const limo_ctx* ctx);
/* Page-locked host memory for buffers that cross PCIe every call (a frame's sweep, a window's observations): every
 * entry point takes pageable or page-locked host pointers alike, page-locked ones are read by the GPU's copy engine
 * directly instead of through the runtime's staging copy.  NULL when the allocation fails. */
void* limo_host_alloc(size_t bytes);
void limo_host_free(void* p);

void limo_ba_default_options(limo_ba_options* out);

/* --- bundle adjustment --------------------------------------------------------------------------- */
/* One window, host buffers in, optimised in place.  = batch_create(1) + solve + download + destroy.
 * The call the reference's node makes per keyframe (mono_lidar.cpp:255).  A window of the common shape (<= 4 free
 * keyframes, one camera each) is solved in ONE cooperative kernel launch (k_solve_coop: several workgroups that meet at
 * device-wide barriers), any other window as a launch sequence - same results bit for bit (KBA_NO_COOP_SOLVE=1 forces
 * the launch sequence).  A wall-clock cap (opts->max_solver_time_sec > 0) is honoured on both paths. */
int limo_ba_solve(limo_ctx* ctx, limo_ba_window* window, const limo_ba_options* opts, limo_ba_report* report);

/*
 * Many independent windows per launch sequence (ragged sizes allowed).  create() packs and uploads;
 * solve() runs entirely from HBM-resident data; reset() restores the uploaded initial parameters on the
 * device (so a batch can be re-solved, e.g. for benchmarking); download() writes the optimised parameters
 * back into the callers' windows (same shapes as at create) and fills n reports (either may be NULL).
 */
int limo_ba_batch_create(limo_ctx* ctx, int32_t n_windows, const limo_ba_window* windows, limo_ba_batch** out);
int limo_ba_batch_solve(limo_ba_batch* batch, const limo_ba_options* opts);
int limo_ba_batch_reset(limo_ba_batch* batch);
int limo_ba_batch_download(limo_ba_batch* batch, limo_ba_window* windows_out, limo_ba_report* reports);
void limo_ba_batch_destroy(limo_ba_batch* batch);
/* Which landmarks of window `window` the trimming rounds of the last solve removed (the outlier groups
 * robust_optimization::solveTrimmed erases, robust_solving.cpp:183-215; the reference only logs their number):
 * removed[l] = 1 for landmark l (the caller's landmark order), else 0.  removed has n_lm entries. */
int limo_ba_batch_trimmed(limo_ba_batch* batch, int32_t window, uint8_t* removed);
/* Device time (ms, HIP events on the batch's stream) and launch count of the Jacobian-evaluation kernel
 * accumulated since create()/the last call with reset != 0; either output may be NULL. */
int limo_ba_batch_kernel_stats(limo_ba_batch* batch, int reset, double* linearize_ms, int64_t* linearize_launches,
                               double* total_ms);
/* Same accumulation window, per timed kernel (the two that dominate an LM iteration). */
#define LIMO_KERNEL_LINEARIZE 0 /* k_lin_lm: residuals + (factored) Jacobians of every observation, landmark blocks */
#define LIMO_KERNEL_SCHUR 1     /* k_schur_lean / k_schur_wide: Schur complement of the landmark blocks (f64 MFMA) */
int limo_ba_batch_kernel_time(limo_ba_batch* batch, int kernel, double* ms, int64_t* launches);

/*
 * Landmark-sharded solve of ONE (large) window, SURVEY §8e / BASELINE.json configs[3]: shard s owns the landmarks
 * whose index in the window satisfies  index mod n_shards == s  together with all their observations and
 * ground-plane rows; camera-side parameters are replicated.  Per LM iteration a shard contributes ONE contiguous block -
 * its camera-side sums per view, its ground-plane rows folded per keyframe (F^T F | F^T r) and the entries of [S | rhs] the
 * camera solve reads (upper triangle of the free slots + rhs): 42 KB for a 10-keyframe / 8000-landmark window - exchanged
 * by ONE all-gather before camera assembly + camera solve (two pieces of it in the first iteration of a solve, where the
 * assembly defines the Jacobi scale the Schur complement needs), and nine doubles by a second all-gather before the step
 * decision; one all-reduce per trimming round and one at the end for the landmarks.  Then every shard factors the reduced
 * camera system redundantly and back-substitutes its own landmarks.  Nothing is summed on the wire: every rank adds the P
 * contributions in shard order, so the result does not depend on how the shards are spread over ranks.
 *   - with a communicator (limo_ctx_comm_init): one process per GPU, shard s lives on rank s mod world (n_shards a
 *     multiple of world, normally == world); every rank calls with the same window; the exchange is an RCCL
 *     all-gather of the blocks (one call per local shard); all ranks return the full result;
 *   - without: n_shards (<= 8) VIRTUAL shards on this GPU - the same kernels, the same blocks, no wire
 *     (the single-GPU mode SURVEY §8e asks for to check the sharding arithmetic).
 * Replaces the same reference call as limo_ba_solve (bundle_adjuster_keyframes.cpp:629-767).
 */
#define LIMO_COMM_ID_BYTES 128
int limo_comm_unique_id(unsigned char id[LIMO_COMM_ID_BYTES]);            /* rank 0; broadcast the bytes to all ranks */
int limo_ctx_comm_init(limo_ctx* ctx, const unsigned char id[LIMO_COMM_ID_BYTES], int rank, int world);
/* The same exchange through a transport of the CALLER instead of RCCL: every exchange step is staged through page-locked host
 * memory and handed to `fn` - kind 0: all-gather (send = count doubles of this rank, recv = world * count doubles in rank order),
 * kind 1: sum over the ranks (send = recv = count doubles).  For ranks that cannot form an RCCL communicator - two processes
 * sharing ONE GPU (a device may appear once per communicator), a host-side fabric - and for tests of the multi-rank branch on a
 * one-GPU box.  fn = NULL removes the transport; limo_ctx_comm_init replaces it. */
typedef void (*limo_exchange_fn)(const double* send, double* recv, long long count, int kind, void* user);
int limo_ctx_comm_init_host(limo_ctx* ctx, limo_exchange_fn fn, void* user, int rank, int world);
int limo_ba_solve_sharded(limo_ctx* ctx, limo_ba_window* window, const limo_ba_options* opts, int n_shards,
                          limo_ba_report* report);
/* Exchange accounting of the last limo_ba_solve_sharded on this context: stats3 = (exchange steps = collective calls with a
 * communicator, counted per local shard; bytes this rank's shards put into them; LM iterations of the solve). */
int limo_ctx_exchange_stats(limo_ctx* ctx, int64_t* stats3);
/* How many one-launch solves (k_solve_coop behind limo_ba_solve / small batches) on this context gave up at a device-wide
 * barrier and were redone as a launch sequence.  A barrier waits at most KBA_COOP_TIMEOUT_MS (default 50) of the GPU's
 * constant clock, which keeps running while a wave is preempted (shared GPU, debugger, profiler); the redo starts from the
 * batch's initial state and gives the same results - the caller never sees an error, this counter is how it can tell. */
int64_t limo_ctx_coop_fallbacks(const limo_ctx* ctx);
/* Which launch path the last limo_ba_batch_solve on this context took - the calls that make and destroy their own batch
 * (limo_ba_solve, limo_ba_adjust_pose_only[_batch], limo_ba_solve_sharded) included.  All paths give the same bits; this is how
 * a test or a profile tells which one it has looked at.
 *   info[0]  path that produced the result: 1 WG (k_solve_wg, one launch, a workgroup per window), 2 COOP (k_solve_coop, one
 *            launch, G workgroups per window), 3 STREAMING (windows move through slots), 4 LOCKSTEP (a launch per phase)
 *   info[1]  1: a cooperative launch gave up at a barrier and the solve was redone through the path of info[0] (see above)
 *   info[2]  G of the cooperative launch that was made (0: none)
 *   info[3]  slot groups and  info[4]  slots of a streaming solve
 *   info[5]  rounds the streaming solve enqueued
 *   info[6]  launches of k_schur_lean_pair (both fast-class Schur lists of a draining round in one launch)
 *   info[7]  the linearisation that ran: 1 k_lin_lm<true> (LDS; also what the one-launch kernels contain), 0 k_lin_lm<false>
 *            (scalar loads: KBA_LIN_VLDS=0, windows with many views) */
int limo_ctx_last_solve_info(const limo_ctx* ctx, int64_t info[8]);
/* Which ground-plane Schur waves the last limo_ba_batch_solve on this context ran (same bits either way; how a test or a profile
 * tells which kernel it has looked at).  A ground-plane group is NARROW when every ground-plane row of its landmarks hangs on one
 * keyframe: its waves build a two-panel tile.  Groups are classified when the batch is packed, and only in a batch whose
 * ground-plane tile has three panels.
 *   info[0]  narrow and  info[1]  wide ground-plane groups of the batch (0, 0: nothing classified)
 *   info[2]  launches of the solve in which narrow groups ran narrow waves (k_schur_lean_gp, k_schur_lean_pair)
 *   info[3]  launches of the solve in which three-panel ground-plane waves ran: for the wide groups, next to the narrow waves in
 *            the same launch; for every group in a batch that classified nothing and under KBA_SCHUR_GP_WIDE=1 (info[2] is 0 then) */
int limo_ctx_last_schur_gp_info(const limo_ctx* ctx, int64_t info[4]);
/* Which form the camera launches (k_cam_assemble, k_cam_solve) of the last limo_ba_batch_solve on this context took: 128 lanes per
 * window or 256, the same bits either way.  The launch sequence picks per launch (128 lanes where the launch lists more windows than
 * 256-lane workgroups fit the device at once, and the batch allows it); KBA_CAM_LANES=128 / 256 forces one form where allowed.  The
 * one-launch paths (info[0] of limo_ctx_last_solve_info 1, 2) count nothing here.
 *   info[0]  launches of k_cam_assemble with 128 lanes,  info[1]  with 256
 *   info[2]  launches of k_cam_solve with 128 lanes,     info[3]  with 256
 *   info[4..7]  workgroups per compute unit at the batch's LDS sizes: k_cam_assemble 128 / 256 lanes, k_cam_solve 128 / 256 lanes
 *   info[8]  windows of the batch whose camera system works in global memory (12 keyframes and up): one of them keeps every camera
 *            launch of the batch at 256 lanes
 * (A call of its own because all eight entries of limo_ctx_last_solve_info are taken; added without an ABI bump, like that one.) */
int limo_ctx_last_cam_lanes_info(const limo_ctx* ctx, int64_t info[9]);

/*
 * Per-iteration solver log: what the reference prints for every solve (minimizer_progress_to_stdout = true,
 * robust_optimization/robust_solving.hpp:105) - Ceres' iteration table, as numbers.  One entry per iteration of every
 * Ceres-style solve of the schedule, recorded on the device by the lane that takes the LM decisions; the same bytes on every
 * launch path (limo_ctx_last_solve_info).  Off by default; switching it on changes no result.
 * An entry exists exactly when Ceres' TrustRegionMinimizer appends an IterationSummary:
 *   - iteration 0 after the first linearisation of a solve: step fields zero, both flags 1, radius = initial_trust_region_radius.
 *     A solve whose first evaluation fails, and a window without a variable parameter block, have no entries;
 *   - an invalid step: cost = the current cost, gradient_max_norm = the previous entry's, step fields zero, the radius after the
 *     division;
 *   - a rejected step: cost = the candidate's cost (+ fixed cost), gradient_max_norm = the previous entry's, the radius after the
 *     division;
 *   - an accepted step: cost and gradient_max_norm of the relinearisation that follows, the radius after the update; no entry
 *     when that relinearisation fails;
 *   - NO entry for an iteration that ends the solve inside the step decision (parameter tolerance, function tolerance, the last
 *     of max_num_consecutive_invalid_steps invalid steps).  limo_ba_report::iterations_total counts such an iteration, the log -
 *     like Ceres' own iteration count - does not: per solve, entries with iteration >= 1 number iterations or iterations - 1;
 *   - a solve ended by the wall-clock cap ends its log where it stood.
 */
typedef struct limo_ba_iteration { /* 64 bytes; ceres::IterationSummary restated */
    int32_t solve;      /* index of the Ceres-style solve inside this call, 0-based, in execution order; a discarded first
                           attempt (robust_solving.cpp:172-181) counts */
    int32_t solve_kind; /* 0 trimming solve, 1 its retry with 3x the iterations, 2 final solve */
    int32_t iteration;  /* 0 = IterationZero */
    uint8_t step_is_valid, step_is_successful, pad[2];
    double cost;        /* incl. the fixed cost, as Ceres reports it */
    double cost_change, gradient_max_norm, step_norm, relative_decrease, trust_region_radius;
} limo_ba_iteration;
/* The switch belongs to the context and is read by limo_ba_batch_solve: when it is on, the solve allocates the log of its batch
 * from the context's pool, with the exact bound of the schedule as the capacity per window:
 *   num_trim_rounds * ((trim_solver_iterations + 1) + (3 * trim_solver_iterations + 1)) + (max_num_iterations + 1)  entries
 * - 111 entries with the default options, about 7 KB per window: 116 MB for a batch of 16384 windows.  Every limo_ba_batch_solve
 * starts the log of its windows at zero entries, limo_ba_batch_reset clears it, and a one-launch solve that gave up at a barrier
 * and was redone (limo_ctx_coop_fallbacks) leaves nothing of the abandoned launch in it. */
int limo_ctx_set_iteration_log(limo_ctx* ctx, int32_t on);
/* The log of window `window` of a resident batch, read on demand: *n = the entries the window has, at most `cap` of them are
 * written to `out` (out == NULL with cap == 0 asks for the count).  With the switch off at the batch's last solve: LIMO_OK, *n = 0. */
int limo_ba_batch_iteration_log(limo_ba_batch* batch, int32_t window, int32_t cap, limo_ba_iteration* out, int32_t* n);
/* The same for the calls that make and destroy their own batch - limo_ba_solve, limo_ba_adjust_pose_only,
 * limo_ba_adjust_pose_only_batch, limo_ba_solve_fixed_landmarks: they copy their windows' logs into a host buffer of the context
 * before they destroy the batch, and this reads window `window` of the last such call.  Switch off: LIMO_OK, *n = 0.
 * Not offered: limo_ba_solve_sharded records no log - after it *n = 0 for every window.
 * Both readers return LIMO_ERR_INVALID (limo_last_error names the argument) for a NULL ctx / batch / n, a window out of range,
 * cap < 0, or out == NULL with cap > 0. */
int limo_ctx_last_iteration_log(limo_ctx* ctx, int32_t window, int32_t cap, limo_ba_iteration* out, int32_t* n);

/*
 * Pose covariance: how well a solve determines its poses - what ceres::Covariance::GetCovarianceBlockInTangentSpace gives for the
 * pose blocks of the problem that has just been solved.  Off by default; switching it on changes no result of a solve.
 * DEFINITION.  For one window, after a solve, J is the Jacobian of the FINAL problem: the problem built at the solve's x0, minus
 * the residual blocks of the landmarks the trimming rounds removed, constant parameter blocks excluded (Ceres' reduced program),
 * evaluated at the final point, robustified (sqrt(rho') folded in, as in every linearisation of the solve), with respect to the
 * tangent parameters of the solve:
 *   rotation 3      delta with q (+) delta = [cos|delta|, sin|delta| delta / |delta|] * q - LEFT-multiplied, rotation ANGLE 2 |delta|:
 *                   a covariance in rotation-vector units is 4 x the rotation-rotation block, 2 x the rotation-translation blocks
 *   translation 3, plane normal 3 (ambient, rank-2 Jacobian), plane distance 1, landmarks 3.
 * The result is the pose-pose block of the generalised inverse of J^T J (landmarks, plane normals and plane distances marginalised).
 * OUTPUT per window: a dense symmetric [6 n_kf][6 n_kf] row-major matrix in the caller's keyframe order, rotation 3 | translation 3
 * per keyframe; rows and columns of keyframes without a free pose block are zero.  An entry and its mirror image are equal bit for
 * bit.  A status per window:
 *   LIMO_COV_OK              the covariance was computed
 *   LIMO_COV_RANK_DEFICIENT  the undamped system is rank deficient beyond the plane normals' own null directions (a free gauge, a
 *                            free keyframe that nothing observes): a Cholesky pivot fell to 2^-26 of its slot's diagonal entry
 *   LIMO_COV_NO_FREE_POSE    the window has no free pose block
 *   LIMO_COV_EVAL_FAILED     the linearisation at the final point failed, or a landmark block did not factor without damping
 *   LIMO_COV_NOT_COMPUTED    the switch was off, or the solve was limo_ba_solve_sharded
 * The matrix is all NaN for every computed status but OK and NO_FREE_POSE, and all zero for NO_FREE_POSE; NOT_COMPUTED has none.
 * COST.  One more linearisation, Schur complement and dense factorisation per window at the end of the solve (six to eight launches), the
 * LM state saved and restored around them: parameters, report, iteration log and trimmed flags of the solve, and every later solve
 * of the batch, are the bytes of a run with the switch off.  With the switch off nothing is launched or allocated.
 */
enum limo_cov_status {
    LIMO_COV_OK = 0,
    LIMO_COV_RANK_DEFICIENT = 1,
    LIMO_COV_NO_FREE_POSE = 2,
    LIMO_COV_EVAL_FAILED = 3,
    LIMO_COV_NOT_COMPUTED = 4
};
/* The switch belongs to the context and is read by every solve on it (limo_ba_batch_solve / _solve_each, and through them
 * limo_ba_solve, limo_ba_solve_fixed_landmarks, limo_ba_adjust_pose_only and its batch forms), on any launch path.  Storage -
 * sum over the windows of (6 n_kf)^2 doubles - comes from the context's pool at the batch's first solve with the switch on. */
int limo_ctx_set_pose_covariance(limo_ctx* ctx, int32_t on);
/* The matrix of window `window` of a resident batch after its last solve: (6 n_kf)^2 doubles into `out` (cap_doubles: the room
 * there; too little is LIMO_ERR_INVALID) and its status.  out == NULL with cap_doubles == 0 asks for the status alone.
 * LIMO_COV_NOT_COMPUTED writes nothing. */
int limo_ba_batch_pose_covariance(limo_ba_batch* batch, int32_t window, int64_t cap_doubles, double* out, int32_t* status);
/* The same for the calls that make and destroy their own batch: window `window` of the last such call on the context. */
int limo_ctx_last_pose_covariance(limo_ctx* ctx, int32_t window, int64_t cap_doubles, double* out, int32_t* status);

/*
 * Evaluate the reprojection / depth residual blocks of a window at its current parameters
 * (Problem::Evaluate semantics).  Outputs are per observation in the caller's observation order; rows
 * 0,1 = reprojection (u,v), row 2 = depth (zero when the observation has no depth):
 *   residuals [n_obs*3]
 *   jac_pose  [n_obs*3*6]  d r / d (rotation tangent 3, translation 3)  — local parameterisation applied
 *   jac_lm    [n_obs*3*3]  d r / d landmark
 *   valid     [n_obs]      0 where the reference functor returns false (|z| < 0.01, cost_functors_ceres.hpp:78-83)
 * apply_loss != 0 applies the Ceres corrector (sqrt(rho') scaling) of the block's loss; cost = 1/2 sum rho.
 * Any output pointer may be NULL.
 */
int limo_ba_evaluate(limo_ctx* ctx, const limo_ba_window* window, const limo_ba_options* opts, int apply_loss,
                     double* cost, double* residuals, double* jac_pose, double* jac_lm, uint8_t* valid);

/* Measurement aid (bench.py `roofline_evaluate`): the same evaluation (apply_loss = 1) over a batch of windows kept on
 * the device, `reps` launches timed with HIP events on the context's stream; nothing is downloaded.
 * device_ms = average time of one launch over all windows. */
int limo_ba_evaluate_batch_time(limo_ctx* ctx, int32_t n_windows, const limo_ba_window* windows, const limo_ba_options* opts,
                                int32_t reps, double* device_ms);

/*
 * Motion-only adjustment of ONE new keyframe against fixed landmarks (adjustPoseOnly).
 * window: n_kf == 1 (the new keyframe; its pose is optimised in place), landmarks constant.
 * Optional speed prior (SpeedRegularizationVector2, cost_functors_ceres.hpp:300-353): enabled when
 * speed_weight > 0: residual (t_new - R_new R_b^T t_b)/dt_cur - vel_prev with pose_before = (q_b,t_b).
 * The call the reference's node makes for every frame (mono_lidar.cpp:203): the whole solveTrimmed schedule of the
 * window runs in ONE kernel launch of one workgroup (k_solve_wg; KBA_NO_WG_SOLVE=1 KBA_NO_COOP_SOLVE=1 force the
 * launch sequence - same bits).
 */
typedef struct limo_speed_prior {
    double speed_weight;     /* 1 - rot_diff/0.03, <= 0 disables (bundle_adjuster_keyframes.cpp:842-843) */
    double dt_cur;           /* seconds                                                                */
    double vel_prev[3];      /* translation(pose_before * pose_before2^-1) / dt_before                  */
    double pose_before[7];
} limo_speed_prior;
int limo_ba_adjust_pose_only(limo_ctx* ctx, limo_ba_window* window, const limo_speed_prior* prior,
                             const limo_ba_options* opts, limo_ba_report* report);

/*
 * N independent adjustPoseOnly problems (each window: n_kf == 1, landmarks constant).  priors: NULL, or n entries;
 * an entry with speed_weight <= 0 means "no prior for this window".
 *   - Window i of a batch gets the result of limo_ba_adjust_pose_only(window i, prior i) BIT FOR BIT: the pose, every
 *     integer of the report, initial_cost and final_cost.  time_sec is the time of the whole batch.
 *   - min_landmarks_for_trimming is the caller's (the reference uses 30 for adjustPoseOnly), as for the single call.  The
 *     resident form takes it from limo_ba_batch_solve(opts), the way limo_ba_batch_create works.
 *   - An invalid window (n_kf != 1, an index out of range, ...) fails the whole call with LIMO_ERR_INVALID; limo_last_error
 *     names the window ("window 3: ...").  n_windows <= 0 and NULL arguments: as limo_ba_batch_create.
 *   - Launch path of a batch of more than one window: ONE launch of k_solve_wg, a workgroup per window, for any N (the
 *     workgroups never wait for each other) when every window has <= 2048 landmarks; otherwise, and under KBA_NO_WG_SOLVE=1,
 *     the lock-step launch sequence - same bits.  Such a batch never streams through slots and never runs k_solve_coop.  A
 *     batch of one window takes the paths of the single call.  The wall-clock cap is honoured per solve on both paths.
 * Resident form: the returned batch is used with limo_ba_batch_solve / _reset / _download / _trimmed / _destroy like any other.
 */
int limo_ba_batch_create_pose_only(limo_ctx* ctx, int32_t n_windows, const limo_ba_window* windows,
                                   const limo_speed_prior* priors, limo_ba_batch** out);
/* create + solve + download + destroy; poses optimised in place, reports[n] may be NULL. */
int limo_ba_adjust_pose_only_batch(limo_ctx* ctx, int32_t n_windows, limo_ba_window* windows, const limo_speed_prior* priors,
                                   const limo_ba_options* opts, limo_ba_report* reports);

/*
 * Per-window solve options: limo_ba_batch_solve / limo_ba_adjust_pose_only_batch with ONE limo_ba_options PER WINDOW - a sweep
 * over outlier-rejection parameters (the reference's tune_parameters_kitti.py: robust_loss_depth_thres x
 * robust_loss_reprojection_thres) runs as one batch instead of one batch per parameter set.  opts has n_opts entries, and n_opts
 * is the number of windows of the batch (n_windows for the pose-only call).
 *   - Fields that may differ from window to window: depth_thres, reprojection_thres, depth_quantile, reprojection_quantile - the
 *     numeric fields of the reference's OutlierRejectionOptions (bundle_adjuster_keyframes.hpp:79-89).  Every other field - the
 *     schedule (num_trim_rounds, trim_solver_iterations, max_num_iterations, max_solver_time_sec), min_landmarks_for_trimming,
 *     minimum_number_residual_groups, the LM constants - must be bitwise equal in all entries.  If one differs the call returns
 *     LIMO_ERR_INVALID before anything is launched and limo_last_error names the first offending window and field ("window 3:
 *     max_num_iterations").  The same for n_opts != the number of windows, opts == NULL, and an entry whose threshold or quantile
 *     is not a finite number ("window 3: depth_thres is not finite").  The batch is untouched and solves normally afterwards.
 *   - Result.  Window i gets the result of the single call (limo_ba_solve / limo_ba_adjust_pose_only /
 *     limo_ba_solve_fixed_landmarks) made with opts[i], BIT FOR BIT: every parameter array, the trimmed set, every integer of the
 *     report, initial_cost and final_cost - on every launch path limo_ctx_last_solve_info can report, with and without the
 *     iteration log.  (The device keeps one 64-byte record per window: the six constants make_consts derives from opts[i]; a
 *     workgroup reads its window's record with one scalar load.)
 *   - No change on the uniform path.  An array whose entries are all equal takes exactly the path of
 *     limo_ba_batch_solve(&opts[0]): no table is uploaded and the kernels see a null table pointer.  A later
 *     limo_ba_batch_solve(opts) on the same batch is uniform again; limo_ba_batch_reset works between the two forms.
 *   - Scope.  Any unsharded batch: limo_ba_batch_create, _create_pose_only, _create_fixed_landmarks.  A landmark-sharded batch
 *     returns LIMO_ERR_INVALID; limo_ba_evaluate* and limo_ba_solve_sharded take one set of options as before.
 */
int limo_ba_batch_solve_each(limo_ba_batch* batch, int32_t n_opts, const limo_ba_options* opts);
/* limo_ba_adjust_pose_only_batch with opts[n_windows]: create + solve_each + download + destroy. */
int limo_ba_adjust_pose_only_batch_each(limo_ctx* ctx, int32_t n_windows, limo_ba_window* windows, const limo_speed_prior* priors,
                                        const limo_ba_options* opts, limo_ba_report* reports);

/*
 * limo_ba_solve with per-landmark constness: the window is solved against landmarks the caller trusts (a map, LiDAR, an older part
 * of the trajectory) - motion-only bundle adjustment over several keyframes, relocalising a short sequence.  What the reference
 * does with BundleAdjusterKeyframes::deactivateLandmarks (bundle_adjuster_keyframes.cpp:221-280; INTEGRATION.md maps its
 * keyframe_fraction onto the flags).
 * lm_fixed: NULL (= limo_ba_solve) or n_lm flags in the caller's landmark order; != 0: the landmark is a constant parameter block
 * (:262-269).
 *   - Problem build.  Everything else is solve()'s: ground rows, scale and ground-plane regularisers, constness of keyframes, the
 *     trimming schedule.  The block counts of the report do not depend on the flags: a constant landmark keeps its residual
 *     blocks, takes part in trimming like any other (limo_ba_batch_trimmed reports it if trimmed) and comes back bit for bit as it
 *     went in.
 *   - Fixed cost.  A residual block without a variable parameter block - a reprojection / depth block, or a ground-height block,
 *     of a LIMO_FIX_POSE keyframe (its plane is fixed with it, :208-216) and a constant landmark - belongs to the fixed cost of
 *     each Ceres-style solve of the schedule: evaluated with its loss at the start of that solve, after the trimming rounds before
 *     it.  initial_cost and final_cost include it; the cost the step acceptance, the function tolerance and every other relative
 *     test see does not (Ceres' reduced program).  This holds for any kf_fixation pattern: the LIMO_FIX_POSE keyframes need not
 *     lead the window.
 *   - Nothing to optimise.  A window whose parameter blocks are all constant returns LIMO_CONVERGENCE with zero iterations and
 *     initial_cost == final_cost == that fixed cost.
 *   - No change without flags.  lm_fixed == NULL, a NULL entry or all-zero flags give the result of limo_ba_solve /
 *     limo_ba_batch_create bit for bit.
 *   - Launch paths.  Window i of a batch gets its single call's result bit for bit, on every launch path
 *     (limo_ctx_last_solve_info).  A window without a variable landmark has no Schur blocks: no Schur kernel runs for it.
 *   - Not offered: limo_ba_solve_sharded takes no flags, and the C++ shim (limo_amd/kba) does not call these two.
 */
int limo_ba_solve_fixed_landmarks(limo_ctx* ctx, limo_ba_window* window, const uint8_t* lm_fixed, const limo_ba_options* opts,
                                  limo_ba_report* report);
/* lm_fixed: NULL, or n_windows entries, each NULL or that window's n_lm flags.  The batch is used with limo_ba_batch_solve / _reset /
 * _download / _trimmed / _destroy like any other; n_windows <= 0 and NULL arguments: as limo_ba_batch_create.  The flags are read
 * during the call only. */
int limo_ba_batch_create_fixed_landmarks(limo_ctx* ctx, int32_t n_windows, const limo_ba_window* windows, const uint8_t* const* lm_fixed,
                                         limo_ba_batch** out);

/*
 * The residual rows of a window that are NOT reprojection / depth blocks, linearised at the window's current parameters the
 * way the solve linearises them (loss corrector / sqrt(weight) applied; Jacobians towards the TANGENT of every parameter block
 * the residual block touches, constant blocks included - the solve masks those later):
 *   LIMO_ROW_GROUND_HEIGHT  GroundPlaneHeightRegularization, cost_functors_ceres.hpp:358-385, wired by
 *                           addGroundPlaneResiduals, bundle_adjuster_keyframes.cpp:517-562 (nearest keyframe, Huber(0.1)
 *                           scaled by 10 (1 - dist / 25)); one row per selected ground landmark that gets a block
 *   LIMO_ROW_SCALE          PoseRegularization, cost_functors_ceres.hpp:229-243, wiring :890-904, weight :704-716
 *   LIMO_ROW_NORMAL_DIFF    VectorDifferenceRegularization (3 rows, sub = component), :775-784
 *   LIMO_ROW_DIST_DIFF      GroundPlaneDistanceRegularization, :786-791
 *   LIMO_ROW_PLANE_MOTION   GroundPlaneMotionRegularization, cost_functors_ceres.hpp:533-547, wiring :794-800
 *   LIMO_ROW_GLOBAL_NORMAL  VectorDifferenceRegularization2 against (0,0,1) (3 rows), :809-816
 *   LIMO_ROW_SPEED          SpeedRegularizationVector2 (3 rows; adjustPoseOnly problem only), cost_functors_ceres.hpp:300-353,
 *                           wiring :835-853
 * kf[0] < kf[1] are the window's keyframe indices the block touches (kf[1] = -1: one keyframe); jac_kf[i] holds the ten
 * tangent slots of kf[i]: rotation 3 | translation 3 | plane normal 3 | plane distance 1.  fixed = 1: every parameter block
 * of the residual block is constant (its cost is part of the fixed cost).  pose_only != 0 builds the adjustPoseOnly problem
 * (window->n_kf == 1, landmarks constant, `prior` as in limo_ba_adjust_pose_only).  Rows come in the order: ground rows
 * (ascending keyframe, then as packed), scale, per consecutive keyframe pair [normal diff x3, dist diff, plane motion],
 * per keyframe global normal x3, speed x3.  *n_rows receives the number of rows of the problem; at most cap are written.
 * The evaluation runs on the device through the same device functions the solve kernels call (gp_lane, reg_row_eval).
 */
enum limo_row_kind {
    LIMO_ROW_GROUND_HEIGHT = 0,
    LIMO_ROW_SCALE = 1,
    LIMO_ROW_NORMAL_DIFF = 2,
    LIMO_ROW_DIST_DIFF = 3,
    LIMO_ROW_PLANE_MOTION = 4,
    LIMO_ROW_GLOBAL_NORMAL = 5,
    LIMO_ROW_SPEED = 6
};
typedef struct limo_ba_row {
    int32_t kind;          /* enum limo_row_kind                                                   */
    int32_t sub;           /* component of a multi-row block                                       */
    int32_t kf[2];         /* window keyframe indices (ascending), kf[1] = -1 if only one          */
    int32_t lm;            /* landmark index in the caller's window (ground rows), else -1         */
    int32_t fixed;         /* 1 = all parameter blocks of the block are constant                   */
    double r;              /* residual, corrector applied                                          */
    double cost;           /* 1/2 rho(|r_block|^2) of the BLOCK, reported on its sub == 0 row      */
    double jac_kf[2][10];  /* d r / d tangent of kf[0], kf[1]                                      */
    double jac_lm[3];      /* d r / d landmark (ground rows)                                       */
} limo_ba_row;
int limo_ba_evaluate_rows(limo_ctx* ctx, const limo_ba_window* window, const limo_speed_prior* prior, int pose_only,
                          const limo_ba_options* opts, int32_t cap, limo_ba_row* rows, int32_t* n_rows);

/* --- landmark initialisation ----------------------------------------------------------------------- */
/*
 * Runs on the device (one lane per landmark, limo_amd/csrc/landmark_init.hip): hand over ALL new landmarks of a
 * keyframe in one call.  ctx is required.
 * For each of n landmarks: rays are given as n_rays_off CSR over (pose_cam_origin [7], u, v, d, f, cx, cy).
 * If the FIRST listed measurement with d >= 0 exists in the landmark's own (newest) keyframe the caller
 * should pass it as mode 0 (depth back-projection, :332-355); else mode 1 = midpoint triangulation over all
 * rays (:358-382; needs >= 2 rays).  ok[i] = 0 where no position could be computed.
 */
typedef struct limo_ray {
    double pose_cam_origin[7]; /* camera <- origin = T_cam_veh * T_kf_origin */
    double f, cx, cy;
    float u, v, d;
    float pad;
} limo_ray;
int limo_landmark_init(limo_ctx* ctx, int32_t n, const int32_t* ray_off /* [n+1] */, const limo_ray* rays,
                       const uint8_t* use_depth /* [n] */, double* pos_out /* [n*3] */, uint8_t* ok /* [n] */);

/* --- trimming --------------------------------------------------------------------------------------- */
/* Quantile trimmer: n (id, value) pairs; outliers = everything from sorted position int(n*q) upwards
 * (ties broken by id so the result is deterministic).  Returns the number of outliers written. */
int limo_trim_quantile(int32_t n, const int64_t* ids, const double* values, double quantile, int64_t* outliers_out);

/* --- LiDAR depth assignment -------------------------------------------------------------------------- */
/* Parameters mirror mono_lidar_fusion_parameters.yaml key by key (defaults = that file; limo_amd/kba/depth_params_yaml.hpp
 * reads the file itself into this struct). */
typedef struct limo_depth_params {
    int32_t pixelarea_search_width;        /* 6   yaml:14 */
    int32_t pixelarea_search_height;       /* 9   yaml:17 */
    int32_t pixelarea_search_offset_x;     /* 0   yaml:21 */
    int32_t pixelarea_search_offset_y;     /* 0   yaml:24 */
    int32_t neighbors_count_min;           /* 3   ours: minimum count of the rectangle search (the file has one for the radius search only, yaml:48) */
    int32_t do_use_histogram_segmentation; /* 1   yaml:58 */
    double histogram_segmentation_bin_width;   /* 0.3 yaml:61 */
    int32_t histogram_segmentation_min_pointcount; /* 1 yaml:63 */
    int32_t treshold_depth_enabled;        /* 1   yaml:97  */
    double treshold_depth_max;             /* 100 yaml:101 */
    double treshold_depth_min;             /* 0   yaml:103 */
    int32_t treshold_depth_local_enabled;  /* 1   yaml:108 */
    int32_t treshold_depth_local_valuetype;/* 1 = relative yaml:112 */
    double treshold_depth_local_value;     /* 0.5 yaml:114 */
    int32_t do_use_cut_behind_camera;      /* 1   yaml:168 */
    int32_t do_use_triangle_size_maximation; /* 1 yaml:171 */
    int32_t do_check_triangleplanar_condition; /* 1 yaml:173 */
    double triangleplanar_crossnorm_treshold;  /* 0.1 yaml:176 */
    double viewray_plane_orthoganality_treshold; /* 0.1 yaml:178 */
    /* ground plane (yaml:125-163) */
    int32_t do_use_ransac_plane;           /* 1   */
    double ransac_plane_distance_treshold; /* 0.2 */
    double ransac_plane_min_z;             /* -3.5 (lidar frame) */
    double ransac_plane_max_z;             /* -1.0 */
    int32_t ransac_plane_max_iterations;   /* 600 */
    double ransac_plane_probability;       /* 0.99 */
    int32_t ransac_plane_use_refinement;   /* 1   */
    double ransac_plane_refinement_treshold;   /* 10.2 */
    double ransac_plane_point_distance_treshold; /* 0.2 */
    int32_t plane_estimator_use_mestimator; /* 1  */
    uint64_t ransac_seed;                  /* ours: RANSAC sampling seed (deterministic) */
    /* ---- ABI 6: the keys of the file the default configuration does not read, in the file's order.  A struct whose
     * fields from here on are all zero selects exactly the path of ABI 5 (rectangle search, largest triangle, rejecting
     * gates, all band returns, weighted / unweighted least-squares patch).  What each mode computes where the file
     * leaves a choice open is written next to the code (limo_amd/csrc/depth.hip, "MODES"). */
    int32_t neighbor_search_mode;          /* 0   yaml:5   0 = rectangle, 1 = search around the feature (below) */
    int32_t do_use_nearestNeighborSearch;  /* 0   yaml:32  mode 1 only; != 0 -> LIMO_ERR_UNSUPPORTED */
    int32_t nnSearch_count;                /* 10  yaml:35  */
    int32_t do_use_radiusSearch;           /* 1   yaml:42  mode 1 only: all visible returns within the radius */
    double radiusSearch_radius;            /* 10  yaml:45  pixels */
    int32_t radiusSearch_count_min;        /* 3   yaml:48  fewer neighbours reject the feature */
    int32_t do_use_depth_segmentation;     /* 0   yaml:74  != 0 -> LIMO_ERR_UNSUPPORTED */
    double depth_segmentation_max_treshold_gradient;                        /* 10   yaml:77 */
    double depth_segmentation_max_neighbor_distance;                        /* 0.2  yaml:79 */
    double depth_segmentation_max_neighbor_distance_gradient;               /* 0.02 yaml:81 */
    double depth_segmentation_max_seedpoint_to_seedpoint_distance;          /* 0.5  yaml:83 */
    double depth_segmentation_max_seedpoint_to_seedpoint_distance_gradient; /* 0.05 yaml:85 */
    double depth_segmentation_max_neighbor_to_seedpoint_distance;           /* 0.5  yaml:87 */
    double depth_segmentation_max_neighbor_to_seedpoint_distance_gradient;  /* 0.05 yaml:89 */
    int32_t depth_segmentation_max_pointcount;                              /* 4    yaml:91 */
    int32_t treshold_depth_mode;           /* 0   yaml:99  1 = a depth outside (min, max) becomes the bound it crossed */
    int32_t treshold_depth_local_mode;     /* 0   yaml:110 the same for the local bounds */
    int32_t do_use_PCA;                    /* 0   yaml:119 patch by PCA; needs do_use_triangle_size_maximation == 0 */
    double pca_debug;                      /* 0.01  yaml:120 accepted, ignored */
    double pca_treshold_3_abs_min;         /* 0.005 yaml:121 largest eigenvalue at least this */
    double pca_treshold_3_2_rel_max;       /* 15    yaml:122 largest <= this * middle */
    double pca_treshold_2_1_rel_min;       /* 1.5   yaml:123 middle >= this * smallest */
    int32_t ransac_plane_use_camx_treshold;/* 0   yaml:145 ground band limited to a corridor in front of the camera */
    double ransac_plane_treshold_camx;     /* 0.2 yaml:147 its FULL width in metres: |x_cam| <= width / 2 */
    int32_t plane_estimator_use_triangle_maximation; /* 0 yaml:153 ground patch = largest triangle of the patch points */
    int32_t plane_estimator_use_leastsquares;        /* 0 yaml:156 ground patch = least squares, weights 1 */
    double plane_estimator_z_x_min_relation;         /* 0 yaml:162 != 0 -> LIMO_ERR_UNSUPPORTED */
    int32_t do_debug_singleFeatures;       /* 0   yaml:183 accepted, ignored */
    int32_t do_publish_points;             /* 0   yaml:184 accepted, ignored */
    int32_t do_depth_calc_statistics;      /* 0   yaml:185 accepted, ignored */
} limo_depth_params;
/* The values of the parameter file.  Settings the library refuses (every depth call, before anything is launched):
 *   LIMO_ERR_UNSUPPORTED  do_use_depth_segmentation != 0; do_use_nearestNeighborSearch != 0 with neighbor_search_mode == 1;
 *                         plane_estimator_z_x_min_relation != 0
 *   LIMO_ERR_INVALID      do_use_PCA together with do_use_triangle_size_maximation; more than one plane_estimator_use_*;
 *                         neighbor_search_mode == 1 with neither search flag set (or a mode other than 0 / 1)
 * limo_last_error names the key. */
void limo_depth_default_params(limo_depth_params* out);

/* Which gate decided a feature (limo_depth_last_reasons).  A feature whose depth a clamping gate (treshold_depth_mode /
 * treshold_depth_local_mode = 1) replaced by a bound carries that gate's code together with a depth. */
enum limo_depth_reason {
    LIMO_DEPTH_OK = 0,          /* a depth was assigned, no gate intervened                        */
    LIMO_DEPTH_NEIGHBOURS = 1,  /* fewer neighbours than neighbors_count_min / radiusSearch_count_min */
    LIMO_DEPTH_HISTOGRAM = 2,   /* no histogram bin is a local maximum with enough points          */
    LIMO_DEPTH_SEGMENT3 = 3,    /* fewer than 3 points in the selected segment                     */
    LIMO_DEPTH_PLANAR = 4,      /* largest triangle fails the planarity gate                       */
    LIMO_DEPTH_PARALLEL = 5,    /* view ray (nearly) parallel to the patch                         */
    LIMO_DEPTH_GLOBAL = 6,      /* global depth gate (rejected, or clamped to treshold_depth_min / _max) */
    LIMO_DEPTH_LOCAL = 7,       /* local depth gate (rejected, or clamped to the local bound)      */
    LIMO_DEPTH_PCA = 8,         /* eigenvalue gates of the PCA patch                               */
    LIMO_DEPTH_DEGENERATE = 9   /* no patch: coincident points                                     */
};

/*
 * Assign a depth to each feature of one frame from one LiDAR sweep.
 *   cloud_xyzi  [n_pts*4] float, KITTI velodyne .bin layout (x,y,z,intensity), lidar frame
 *   T_cam_lidar [7]       camera <- lidar
 *   feat_uv     [n_feat*2] float pixel coordinates
 *   feat_is_ground [n_feat] optional (NULL = none): features labelled as ground use the ground-plane path
 *   depth_out   [n_feat]  metres along camera z, -1 where no depth could be assigned
 */
int limo_depth_estimate(limo_ctx* ctx, const float* cloud_xyzi, size_t n_pts, const double* T_cam_lidar,
                        double f, double cx, double cy, int32_t img_w, int32_t img_h, const float* feat_uv,
                        size_t n_feat, const uint8_t* feat_is_ground, const limo_depth_params* params,
                        float* depth_out);

/*
 * The same call in two halves, so that a frame's depth assignment runs on the GPU while the host thread is busy with something
 * else (the reference runs the depth estimator as a process of its own beside the bundle-adjustment node:
 * demo_keyframe_bundle_adjustment_meta/launch/kitti_standalone.launch:14-23 the `tracklet_depth_node`, :55 the BA node - the two overlap there too):
 *   limo_depth_estimate_begin  enqueues the copies and the kernels on the context's stream and returns; cloud_xyzi must stay
 *                              valid until _end (from limo_host_alloc memory the copy is a DMA, from pageable memory the runtime
 *                              stages it before returning); feat_uv / feat_is_ground are consumed before it returns
 *   limo_depth_estimate_end    waits for that work and writes depth_out[n_feat] (n_feat of the _begin call)
 * One call may be open per context: _begin with one open, or _end (or any other depth call) out of order -> LIMO_ERR_INVALID.
 * limo_depth_estimate is exactly _begin followed by _end.
 */
int limo_depth_estimate_begin(limo_ctx* ctx, const float* cloud_xyzi, size_t n_pts, const double* T_cam_lidar,
                              double f, double cx, double cy, int32_t img_w, int32_t img_h, const float* feat_uv,
                              size_t n_feat, const uint8_t* feat_is_ground, const limo_depth_params* params);
int limo_depth_estimate_end(limo_ctx* ctx, float* depth_out, size_t n_feat);

/*
 * The same for a batch of sweeps of one sensor rig (an offline replay: the reference's demo application reads every
 * frame of a KITTI sequence from disk, demo_keyframe_bundle_adjustment_meta/apps/main_program/main_program.cpp:97-170):
 * the frame is a grid dimension of every kernel, so a call costs seven launches whatever n_frames is.  Results are
 * those of n_frames separate limo_depth_estimate calls, bit for bit.
 *   flags & LIMO_DEPTH_DEVICE_POINTERS: cloud_xyzi / feat_uv / feat_is_ground / depth_out of every frame are device
 *   pointers on the context's GPU (sweeps already resident in HBM; nothing is copied).  A non-NULL feat_is_ground then
 *   means "estimate the ground plane of this frame" (the labels cannot be inspected from the host).
 */
typedef struct limo_depth_frame {
    const float* cloud_xyzi;       /* [n_pts*4]  */
    size_t n_pts;
    const float* feat_uv;          /* [n_feat*2] */
    size_t n_feat;
    const uint8_t* feat_is_ground; /* [n_feat] or NULL */
    float* depth_out;              /* [n_feat]   */
} limo_depth_frame;
#define LIMO_DEPTH_DEVICE_POINTERS 1u
int limo_depth_estimate_batch(limo_ctx* ctx, int32_t n_frames, const limo_depth_frame* frames, const double* T_cam_lidar,
                              double f, double cx, double cy, int32_t img_w, int32_t img_h, const limo_depth_params* params,
                              uint32_t flags);

/*
 * Ground plane of frame `frame` of the LAST limo_depth_estimate / limo_depth_estimate_batch launch group on this context
 * (a batch call runs groups of 32 frames; `frame` counts inside the last group): plane4 = (n, d) with n.p + d = 0 in the
 * camera frame, d >= 0; all zero and *inliers = 0 if the frame had no ground-labelled feature or no plane was found.
 * The estimator computes this plane anyway (yaml:125-143); the accessor exists so that a caller - and the parity tests -
 * can look at it.
 */
int limo_depth_last_ground_plane(limo_ctx* ctx, int32_t frame, double* plane4, int32_t* inliers /* may be NULL */);
/*
 * The gate that decided each feature of frame `frame` of the last launch group (enum limo_depth_reason, one byte per
 * feature; n_feat = that frame's feature count).  Counting them answers "which gate starves my workload of depths".
 */
int limo_depth_last_reasons(limo_ctx* ctx, int32_t frame, uint8_t* reasons, size_t n_feat);
/*
 * Measurement aid (bench.py `roofline_depth`): with timing on, every launch group records HIP events on the context's
 * stream around its kernels; limo_depth_last_kernel_ms returns the device time of the last group in milliseconds:
 * ms4 = (k_project, ground-plane kernels k_ransac / k_pick / k_refine / k_plane, k_features, their sum).
 */
int limo_depth_set_timing(limo_ctx* ctx, int32_t on);
int limo_depth_last_kernel_ms(limo_ctx* ctx, double* ms4);

/* --- five-point motion prior ------------------------------------------------------------------------- */
/*
 * Relative camera motion from image correspondences alone: the prior the node computes for every frame that arrives
 * without a tf prior (helpers::getMotionUnscaled called at keyframe_bundle_adjustment_ros_tool/src/mono_lidar/
 * mono_lidar.cpp:156-162 and mono_standalone.cpp:112).  Replaces calcMotion5Point,
 * src/commons/general_helpers.hpp:103-140: cv::findEssentialMat(points1, points0, focal, pp, RANSAC, probability, 2.0)
 * (:122) + cv::recoverPose (:129); the mean-flow gate (:112-121) and getMotionUnscaled's scaling and frame changes
 * (:209-231) stay with the caller (limo_amd/kba/five_point.hpp:matches / meanFlow / motionUnscaled).
 * Runs on the device (limo_amd/csrc/five_point.hip): every minimal sample of a round at once, every model scored against
 * every match, the adaptive stopping rule applied afterwards on the host.  The result is the one of the host estimator
 * limo_amd/kba/five_point.hpp:estimateMotion for the same inputs and seed, BIT FOR BIT (limo_amd/csrc/five_point_core.hpp).
 */
typedef struct limo_five_point_params {
    double probability;    /* 0.999  general_helpers.hpp:221 (getMotionUnscaled's argument to calcMotion5Point) */
    double threshold_px;   /* 2.0    general_helpers.hpp:122 (last argument of cv::findEssentialMat) */
    int32_t max_samples;   /* 1000   cv::findEssentialMat's RANSAC iteration cap; 1 .. 16384 */
    int32_t chunk;         /* 0 = the library's schedule; > 0: samples per device round.  No result depends on it */
} limo_five_point_params;
typedef struct limo_five_point_motion { /* five_point::Motion; what calcMotion5Point hands back through cv::recoverPose (:129-139) */
    int32_t ok, inliers, in_front, samples;
    double E[9], R[9], t[3];            /* row-major; x_b = R x_a + t, |t| = 1; b^T E a = 0 */
} limo_five_point_motion;
typedef struct limo_five_point_frame { /* helpers::getMatches' two point lists (general_helpers.hpp:35-74) */
    int32_t n;
    const double* pts_a;               /* [n*2] pixels */
    const double* pts_b;               /* [n*2] pixels */
    uint64_t seed;                     /* of the sample picks (OpenCV draws from its global RNG) */
} limo_five_point_frame;
/* the values calcMotion5Point is called with (general_helpers.hpp:122, :221) */
void limo_five_point_default_params(limo_five_point_params* out);
/*
 * One pair of frames (general_helpers.hpp:122-129).  n < 5, or no sample giving a model: LIMO_OK with ok = 0, R = I,
 * t = (0, 0, 1).  NULL pointers, n < 0, a non-finite coordinate or an out-of-range parameter: LIMO_ERR_INVALID.
 * inlier: the mask cv::findEssentialMat returns (:122 `mask`), one byte per match, or NULL.
 */
int limo_five_point(limo_ctx* ctx, const limo_five_point_frame* frame, double focal, double cx, double cy,
                    const limo_five_point_params* params, limo_five_point_motion* out, uint8_t* inlier /* [n] or NULL */);
/*
 * The same for n_frames pairs of one camera (an offline replay; N sequences in lock step): the frame is a grid dimension of
 * every kernel, a frame whose stopping rule has fired takes no part in later rounds.  out[i] holds the bytes of frame i's
 * single call.  limo_last_error names the frame an error belongs to.
 */
int limo_five_point_batch(limo_ctx* ctx, int32_t n_frames, const limo_five_point_frame* frames, double focal, double cx, double cy,
                          const limo_five_point_params* params, limo_five_point_motion* out /* [n_frames] */);

/* --- landmark selection ------------------------------------------------------------------------------ */
/*
 * Which landmarks of the window enter the next solve: the selector the node runs in front of every solve()
 * (keyframe_bundle_adjustment/src/bundle_adjuster_keyframes.cpp:118 cheirality rejection, always first; the schemes
 * keyframe_bundle_adjustment_ros_tool/src/mono_lidar/mono_lidar.cpp:396-430 adds: voxel sparsification :396-408 and "depth
 * assurance" :409-426; the union is LandmarkSelector::select, include/keyframe_bundle_adjustment/landmark_selector.hpp:118-253).
 *   rejection       landmark_selection_scheme_cheirality.cpp:22-60: dropped iff behind some camera that measured it
 *   sparsification  landmark_selection_scheme_voxel.cpp:116-233: frame of the newest keyframe, z in [-20, 100], distance to the driven
 *                   path (far / middle pipe), one representative per voxel, budgets: near = largest image flow, middle = hashed
 *                   rank seeded with the newest stamp, far = seen by the most keyframes; ties go to the smaller id
 *   must-haves      landmark_selection_scheme_add_depth.cpp:16-76: per entry the `count` landmarks that pass the predicate, are
 *                   measured in the active keyframe of time rank frame_index and have the smallest key (then id)
 * Runs on the device (limo_amd/csrc/landmark_select.hip).  The bytes are those of the host classes limo_amd/kba/landmark_selector.hpp
 * + landmark_selection_voxel.hpp compiled with floating-point contraction off (limo_amd/csrc/landmark_select_core.hpp states the
 * arithmetic once for both).  Outlier removal and the "unselected" bookkeeping of LandmarkSelector stay with the caller.
 * A pool whose voxel indices leave (-2^20, 2^20) (e.g. a voxel size of 1e-5 m) is finished on the host with the same statement.
 * Limits: n_kf <= 64, n_cam <= 8 (LIMO_ERR_INVALID beyond; the shim then uses its host selector).
 */
enum { LIMO_SELECT_HAS_DEPTH = 0, LIMO_SELECT_IS_GROUND = 1 };           /* predicate: Landmark::has_measured_depth / is_ground_plane */
enum { LIMO_SELECT_KEY_MEASURED_DEPTH = 0, LIMO_SELECT_KEY_RANGE = 1 };  /* key, smallest win: (double)m.d / (double)(float)|T_kf p| (mono_lidar.cpp:412-423) */
typedef struct limo_select_add { int32_t frame_index, count, predicate, key; } limo_select_add;
typedef struct limo_select_params {
    double voxel_size_xyz[3];      /* 0.5 0.5 0.3  mono_lidar.cpp:404 */
    double roi_far, roi_middle;    /* 40, 15       mono_lidar.cpp:405-408 */
    uint32_t max_near, max_middle, max_far;   /* 200 200 100  keyframe_ba_monolid.launch:36-38 */
    int32_t n_add; const limo_select_add* add;
    int32_t sort_capacity;         /* 0 = the library's; > 0: landmarks the on-chip sort takes before the global-memory path.  No result depends on it */
} limo_select_params;
typedef struct limo_select_pool {  /* active keyframes ascending keyframe id, candidate landmarks ascending id */
    int32_t n_kf, n_cam, n_lm, n_obs;
    const double* kf_pose;         /* [n_kf*7]   as limo_ba_window */
    const uint64_t* kf_stamp;      /* [n_kf]     */
    const double* cam;             /* [n_cam*10] as limo_ba_window */
    const uint64_t* lm_id;         /* [n_lm] strictly ascending */
    const double* lm_pos;          /* [n_lm*3]   */
    const uint8_t* lm_has_depth;   /* [n_lm]     */
    const uint8_t* lm_is_ground;   /* [n_lm]     */
    const int32_t *obs_kf, *obs_lm, *obs_cam; const float *obs_u, *obs_v, *obs_d;  /* [n_obs] any order, each (kf, lm, cam) once */
} limo_select_pool;
/* the node's wiring (mono_lidar.cpp:404-408, launch :36-38); its must-have list needs the window size: n_add = 0 here */
void limo_select_default_params(limo_select_params* out);
/*
 * out[i]: low two bits 0 = not chosen by the voxel scheme, 1 = near, 2 = middle, 3 = far field; | 4 = must-have; 8 = rejected by
 * cheirality (nothing else set).  Selected iff out[i] & 7.  n_kf == 0 or n_lm == 0: LIMO_OK, out all zero.  Non-finite landmark
 * positions are no error (the comparisons decide, as on the host).  LIMO_ERR_INVALID (limo_last_error names pool and field), before
 * anything is launched: NULL pointers, negative sizes, an index out of range, lm_id not strictly ascending, a (kf, lm, cam) twice,
 * a non-positive voxel size or roi, an unknown predicate or key, n_kf > 64, n_cam > 8.
 */
int limo_landmark_select(limo_ctx* ctx, const limo_select_pool* pool, const limo_select_params* params, uint8_t* out /* [n_lm] */);
/* The same for n_pools windows (N sequences in lock step): the pool is a grid dimension of every kernel, three launches whatever
 * n_pools is.  out[p] holds the bytes of pool p's single call. */
int limo_landmark_select_batch(limo_ctx* ctx, int32_t n_pools, const limo_select_pool* pools, const limo_select_params* params,
                               uint8_t* const* out);
/* Measurement aid (scripts/bench_landmark_select.py): with timing on, HIP events are recorded around the three kernels of a call;
 * limo_select_last_kernel_ms returns the device time of the last call in milliseconds. */
int limo_select_set_timing(limo_ctx* ctx, int32_t on);
int limo_select_last_kernel_ms(limo_ctx* ctx, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* LIMO_HIP_H_ */
