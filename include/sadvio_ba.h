/*
 * sadvio_ba.h — C ABI of the MI355X-native sliding-window bundle-adjustment backend.
 *
 * This is the drop-in boundary for SaDVIO's optimizer hot path. Every entry point names the
 * reference interface it replaces (paths relative to the reference checkout, `cpp/...`).
 * The reference has no FFI of its own (100 % C++); what a maintainer binds is
 * an `isae::AOptimizer` subclass that flattens the object graph into `sadvio_flat_window`,
 * calls these functions and applies the returned *deltas* with the reference's own
 * composition rules (AOptimizer.cpp:329-340,391-434). See INTEGRATION.md.
 *
 * Conventions
 *   - All floating point is IEEE FP64 (the reference is FP64 throughout).
 *   - A rigid transform is 12 doubles: R row-major (9) followed by t (3).
 *     `T_f_w` = world->frame (frame.h:48-51), `T_s_f` = frame->sensor (ASensor.h:43-44).
 *   - Optimisation variables are deltas initialised to zero and composed on the right:
 *     T_f_w = T_f_w0 * (exp(w), t)  (geometry.h:198-203; parametersBlock.hpp:34-37 — NOT the
 *     SE3 exponential), p = p0 + dl (geometry.h:205-210).
 *   - Return value 0 = OK, negative = SADVIO_E_*; nothing throws across the boundary.
 *   - A handle owns one HIP stream and all device mirrors; it is not re-entrant. Two handles
 *     (front-end / back-end optimizer instances, slamParameters.cpp:273-275) may be used
 *     concurrently from different host threads.
 *   - The library has NO CPU fallback: every compute entry point fails with
 *     SADVIO_E_NO_DEVICE / SADVIO_E_HIP when no gfx950 device is usable.
 */
#ifndef SADVIO_BA_H
#define SADVIO_BA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SADVIO_OK 0
#define SADVIO_E_INVALID_ARG (-1)
#define SADVIO_E_NOT_USABLE (-2) /* solver produced no usable solution (AOptimizer.cpp:259) */
#define SADVIO_E_HIP (-3)
#define SADVIO_E_RCCL (-4)
#define SADVIO_E_NO_DEVICE (-5)
#define SADVIO_E_STATE (-6)   /* call order violated (e.g. solve before set_window) */
#define SADVIO_E_REFUSED (-7) /* marginalisation refused: n < 4 (marginalization.cpp:215-216) */

/* Visual factor flavour of a window. */
#define SADVIO_FACTOR_PIXEL 0   /* ReprojectionErrCeres_pointxd_dx, BundleAdjustmentCERESAnalytic.h:41-98 */
#define SADVIO_FACTOR_ANGULAR 1 /* AngularErrCeres_pointxd_dx, AngularAdjustmentCERESAnalytic.h:45-120 */

/* Termination codes in sadvio_solve_summary.termination (Ceres TerminationType semantics). */
#define SADVIO_TERM_NO_CONVERGENCE 0 /* max_num_iterations reached */
#define SADVIO_TERM_FUNCTION_TOL 1
#define SADVIO_TERM_PARAMETER_TOL 2
#define SADVIO_TERM_GRADIENT_TOL 3
#define SADVIO_TERM_MIN_RADIUS 4
#define SADVIO_TERM_FAILURE 5 /* too many consecutive invalid steps */

typedef struct sadvio_ba_handle sadvio_ba_handle;

typedef struct sadvio_ba_config {
    int32_t device;          /* HIP device ordinal */
    int32_t profile_kernels; /* 1: bracket every kernel class with hipEvents (see get_kernel_times) */
    int32_t use_graph;       /* 1: replay the iteration sequence from a captured hipGraph */
    int32_t reserved;        /* flags; 0 = none. SADVIO_CFG_LONG_TRACKS: accept landmarks with more than 64 observations (see sadvio_flat_window);
                                SADVIO_CFG_LONG_TRACK_PRIORS: ... and marginalise, sparsify and hold them under priors;
                                SADVIO_CFG_LONG_TRACK_COVARIANCE: ... and serve covariances of windows that hold them. A refused combination:
                                SADVIO_E_INVALID_ARG, the text through sadvio_ba_last_error(NULL) */
} sadvio_ba_config;
#define SADVIO_CFG_LONG_TRACKS 1
#define SADVIO_CFG_LONG_TRACK_PRIORS 2 /* with SADVIO_CFG_LONG_TRACKS: marginalize, sparsify and the prior setters serve long tracks */
#define SADVIO_CFG_LONG_TRACK_COVARIANCE 4 /* with SADVIO_CFG_LONG_TRACKS: sadvio_ba_covariance and _covariance_cross serve windows with long tracks */
#define SADVIO_CFG_LONG_TRACK_BATCH 8 /* with SADVIO_CFG_LONG_TRACKS: sadvio_ba_marginalize_relative and _relative_batch serve windows with long tracks; with SADVIO_CFG_LONG_TRACK_COVARIANCE as well, sadvio_ba_covariance_batch */

/*
 * One sliding window, flattened (SoA, index based). Replaces the object-graph walk of
 * BundleAdjustmentCERESAnalytic::addResidualsLocalMap (BundleAdjustmentCERESAnalytic.cpp:197-314)
 * / AngularAdjustmentCERESAnalytic::addResidualsLocalMap (…Angular….cpp:212-339).
 * Inclusion rules the flattener must apply (the adapter side owns them):
 *   - key-frames in the order of LocalMap::getLastNFramesIn, newest first (amap.h:28-32);
 *     kf_const[i] = 1 iff i > n_kf - fixed - 1 (…Analytic.cpp:219);
 *   - landmark included iff isInitialized && !isOutlier (…Analytic.cpp:239);
 *   - observation included iff its sensor's frame is a key-frame of the window (…Analytic.cpp:256-258).
 * Observations are CSR by landmark. All arrays are caller-owned; set_window copies them.
 *
 * Observations per landmark. A handle created with sadvio_ba_config.reserved = 0 takes at most 64 observations per landmark and
 * refuses the window otherwise ("a landmark has more than 64 observations"), as every handle always did: callers that rely on that
 * refusal keep it. A handle created with SADVIO_CFG_LONG_TRACKS takes any number of observations up to SADVIO_MAX_LONG_TRACK_OBS, from
 * up to SADVIO_MAX_LONG_TRACK_KF distinct key-frames. Landmarks of at most 64 observations are solved in the landmark tiles; one with
 * more is a LONG TRACK: inside the same LM step it is linearised, eliminated and back-substituted by kernels of its own (DESIGN.md
 * "Long tracks"), and its index and its place in every output array are what they would be anyway. On a handle with that flag
 * alone a long track is free or constant, carries real observations only and cannot be kept in the reduced system: see
 * set_dense_prior / set_sparse_priors, and the calls that refuse a window holding one (sadvio_ba_covariance*, sadvio_ba_marginalize*,
 * sadvio_ba_sparsify naming one), all with SADVIO_E_INVALID_ARG and a text that names long tracks: callers that rely on those
 * refusals keep them.
 *
 * Long tracks under a prior. A handle created with SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_PRIORS steps a sliding window that
 * holds long tracks (SADVIO_CFG_LONG_TRACK_PRIORS without SADVIO_CFG_LONG_TRACKS: sadvio_ba_create fails with SADVIO_E_INVALID_ARG):
 *   - sadvio_ba_marginalize takes a window with long tracks; one may stand in lmk_keep or lmk_marg;
 *   - sadvio_ba_sparsify takes a long track among its kept landmarks;
 *   - sadvio_ba_set_dense_prior keeps a long track in the reduced system like any landmark (3 columns behind the poses);
 *   - sadvio_ba_set_sparse_priors: a landmark-prior or landmark-to-landmark factor holds its long track in the reduced system; a
 *     pose-to-landmark factor on a free long track HOLDS it there too (on a landmark of the tiles such a factor rides the
 *     elimination as two pseudo-observations; a long track carries real observations only, with or without this flag).
 *   A held long track costs what any held landmark costs: 3 more columns of the reduced system in every LM step, and one thread
 *   per observation of it adding its rows (k_build_kept); its pose-pose part is still summed by the long kernels.
 *   sadvio_ba_covariance, _covariance_batch, _covariance_cross, sadvio_ba_marginalize_relative and _relative_batch refuse a window
 *   with long tracks as before, with this flag or without it (the two flags below lift those refusals).
 *
 * Covariances of windows with long tracks. A handle created with SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_COVARIANCE (without
 * SADVIO_CFG_LONG_TRACKS: sadvio_ba_create fails with SADVIO_E_INVALID_ARG, the text through sadvio_ba_last_error(NULL)) serves
 * sadvio_ba_covariance and sadvio_ba_covariance_cross on a window that holds long tracks: both assemblies (SADVIO_COV_SQRT), both
 * routes (dense, band) and the retry, with the bit guarantees of those calls. A long track's landmark block, its cross blocks and the
 * innovation of a candidate observation of it are what they are for any landmark: eliminated, constant (zeros), or — together with
 * SADVIO_CFG_LONG_TRACK_PRIORS — kept in the reduced system by a prior. The flag is independent of SADVIO_CFG_LONG_TRACK_PRIORS
 * (reserved = 1 | 4 and 1 | 2 | 4 are both valid). A handle without it keeps every refusal above with the same text. With it alone,
 * sadvio_ba_covariance_batch, sadvio_ba_marginalize_relative and sadvio_ba_marginalize_relative_batch still refuse a window with
 * long tracks, with the same text. On any handle a window without long tracks takes the launches it always took and returns the
 * same bits. DESIGN.md "Covariances of windows with long tracks".
 *
 * Batch calls on windows with long tracks. A handle created with SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_BATCH (without
 * SADVIO_CFG_LONG_TRACKS: sadvio_ba_create fails with SADVIO_E_INVALID_ARG, the text through sadvio_ba_last_error(NULL)) serves
 * sadvio_ba_marginalize_relative and sadvio_ba_marginalize_relative_batch on a window that holds long tracks: a long track shared by
 * the two key-frames is an item like any landmark, with the multiplicity, the cuts and the bits a walk over all its observations
 * would give (its observations in the two key-frames are found by bisection). With SADVIO_CFG_LONG_TRACK_COVARIANCE as well
 * (reserved = 1 | 4 | 8, or 1 | 2 | 4 | 8) sadvio_ba_covariance_batch serves such windows on every route, with the guarantees stated
 * at that call; with SADVIO_CFG_LONG_TRACK_BATCH but without SADVIO_CFG_LONG_TRACK_COVARIANCE it keeps refusing, with the same text
 * (its DENSE and BAND items, its retry and its SADVIO_COV_SQRT=1 items go through the steps of sadvio_ba_covariance, which that flag
 * gates). A handle without SADVIO_CFG_LONG_TRACK_BATCH keeps all three refusals, text unchanged. After this, no call on a window
 * held by one GPU refuses it for a long track on a handle with reserved = 1 | 2 | 4 | 8. DESIGN.md "Batch calls on windows with
 * long tracks".
 * A window sharded over several GPUs has no long path: it is refused at 65 observations whatever the flags. On a handle with the flag, SADVIO_LONG_MIN in the environment (read by sadvio_ba_create; an
 * integer in [2, 65], default 65; tests and A/B timing) sends every landmark with at least that many observations down the long path.
 */
#define SADVIO_MAX_LONG_TRACK_OBS 4096 /* observations of one landmark */
#define SADVIO_MAX_LONG_TRACK_KF 512   /* distinct key-frames observing one landmark with more than 64 observations */
typedef struct sadvio_flat_window {
    int32_t n_kf;
    int32_t n_cam;
    int32_t n_lmk;
    int32_t n_obs;
    int32_t factor_type; /* SADVIO_FACTOR_* */
    int32_t has_imu;     /* 1: every key-frame carries (v, ba, bg) states (AOptimizer.cpp:29-53) */

    const int64_t *kf_id;    /* [n_kf] opaque ids, echoed unchanged (frame.h:21-22) */
    const double *kf_T_f_w;  /* [n_kf][12] */
    const uint8_t *kf_const; /* [n_kf] */
    const double *kf_vel;    /* [n_kf][3] or NULL (IMU.h:77-100) */
    const double *kf_ba;     /* [n_kf][3] or NULL */
    const double *kf_bg;     /* [n_kf][3] or NULL */

    const double *cam_K;     /* [n_cam][4] fx fy cx cy (ASensor.cpp:17) */
    const double *cam_T_s_f; /* [n_cam][12] (ASensor.h:44) */
    const double *cam_sigma; /* [n_cam] measurement sigma: 1.0 pixel (…Analytic.h:46);
                                1.5/f angular window BA (…Angular….cpp:283) */

    const int64_t *lmk_id;      /* [n_lmk] opaque ids, echoed unchanged (ALandmark.h:18-19) */
    const double *lmk_p;        /* [n_lmk][3] T_w_lmk.translation() (ALandmark.h:36-39) */
    const uint8_t *lmk_const;   /* [n_lmk] or NULL = all free */
    const int32_t *lmk_obs_ptr; /* [n_lmk+1] CSR offsets into obs_* */
    const int32_t *obs_kf;      /* [n_obs] index into kf_* */
    const int32_t *obs_cam;     /* [n_obs] index into cam_* */
    const double *obs_meas;     /* [n_obs][2] pixel uv (AFeature2D.h:21) | [n_obs][3] unit bearing (AFeature2D.h:80) */
} sadvio_flat_window;

/*
 * Line landmarks ("linexd": Line3D with ModelLine3D, Line3D.h:8-36, Model3D.h:45-51) of one window — SURVEY.md §8f rank 3.
 * A line is a 6-dof pose parameter block, T_w_l <- T_w_l (exp(w), t) (PoseParametersBlock; write-back AOptimizer.cpp:334-336),
 * observed as a 2-D segment. Residual blocks, added by addResidualsLocalMap for every feature whose frame is a key-frame of
 * the window (BundleAdjustmentCERESAnalytic.cpp:273-311 / AngularAdjustmentCERESAnalytic.cpp:293-333):
 *   pixel windows    ReprojectionErrCeres_linexd_dx (…Analytic.h:102-195): the two model points projected with
 *                    Camera::project against the two measured end points, 4 residuals, sigma 1. As coded the landmark is
 *                    moved by T_w_l (I, x[0..2]) — the first three entries of its 6-vector, used as a TRANSLATION — while the
 *                    Jacobian treats them as a rotation ([-R [pt]x | I]); reproduced. The cost-only branch of the reference
 *                    (:168-177) reads an uninitialised projection: the residual of the Jacobian branch is used for both.
 *   angular windows  AngularErrCeres_linexd_dx (…Angular….h:368-469): coplanarity of the observation plane (b0 x b1) with
 *                    the line, 2 residuals, weight 1 / sigma^2 with sigma 1.
 * Lines stay in the reduced system (6 columns each after the key-frames and the prior-kept landmarks): they are few.
 */
typedef struct sadvio_line_set {
    int32_t n_line, n_obs;
    const int64_t *line_id;      /* [n_line] opaque ids, echoed */
    const double *line_T_w_l;    /* [n_line][12] landmark->getPose() */
    const double *line_model;    /* [n_line][6] the two model points (ModelLine3D: (-0.5, 0, 0), (0.5, 0, 0)) */
    const uint8_t *line_const;   /* [n_line] or NULL */
    const int32_t *line_obs_ptr; /* [n_line + 1] CSR */
    const int32_t *obs_kf;       /* [n_obs] */
    const int32_t *obs_cam;      /* [n_obs] */
    const double *obs_meas;      /* pixel: [n_obs][4] end points (AFeature::getPoints) | angular: [n_obs][6] two bearings */
} sadvio_line_set;

/* Constants of one IMUFactor + IMUBiasFactor pair (residuals.hpp:133-300); pairing rule
 * AOptimizer::addIMUResiduals (AOptimizer.cpp:55-92): consecutive KFs, dt <= 1 s. kf_i is the
 * older frame (imu_j->getLastKF()). All 3x3 are row-major. */
typedef struct sadvio_imu_factor {
    int32_t kf_i, kf_j;
    double dt;            /* (ts_j - ts_i) * 1e-9 */
    double delta_R[9];    /* IMU::getDeltaR of imu_j */
    double delta_v[3];
    double delta_p[3];
    double J_dR_bg[9];    /* IMU.h:141-145 */
    double J_dv_ba[9];
    double J_dv_bg[9];
    double J_dp_ba[9];
    double J_dp_bg[9];
    double cov[81];       /* IMU::getCov of imu_j, 9x9 row-major */
    double bacc_noise;    /* imu_i->getbAccNoise() (residuals.hpp:259) */
    double bgyr_noise;    /* imu_i->getbGyrNoise() (residuals.hpp:261) */
} sadvio_imu_factor;

/* PosePriordx (residuals.hpp:601-632); sqrt_inf = diag(inf_diag) (…Analytic.cpp:226). */
typedef struct sadvio_pose_prior {
    int32_t kf;
    int32_t pad;
    double T_prior[12];
    double inf_diag[6];
} sadvio_pose_prior;

/* One factor of the sparsified (NFR) marginalisation prior, added by the sparse branch of
 * addMarginalizationResiduals (BundleAdjustmentCERESAnalytic.cpp:363-426). Every landmark such a factor touches
 * stays in the reduced system (it is coupled to other variables than its own observations).
 *   SADVIO_SPARSE_IMU_PRIOR      IMUPriordx               (residuals.hpp:649-695)  kf; T_prior, v/ba/bg_prior, sqrt_inf 15x15
 *   SADVIO_SPARSE_POSE_TO_LMK    PoseToLandmarkFactor     (residuals.hpp:570-595)  kf, lmk0; delta, sqrt_inf 3x3
 *   SADVIO_SPARSE_LMK_PRIOR      Landmark3DPrior          (residuals.hpp:512-522)  lmk0; delta = prior, sqrt_inf 3x3
 *   SADVIO_SPARSE_LMK_TO_LMK     LandmarkToLandmarkFactor (residuals.hpp:537-556)  lmk0, lmk1; delta, sqrt_inf 3x3
 * The linearisation-point values the reference copies into the factor (_T, _v, _ba, _bg, _lmk, _t_w_lmk) are the
 * window's own kf_* / lmk_p entries. sqrt_inf is row-major; 3x3 matrices use the first 9 entries. */
#define SADVIO_SPARSE_IMU_PRIOR 0
#define SADVIO_SPARSE_POSE_TO_LMK 1
#define SADVIO_SPARSE_LMK_PRIOR 2
#define SADVIO_SPARSE_LMK_TO_LMK 3
/*   SADVIO_SPARSE_RELATIVE_POSE  Relative6DPose           (residuals.hpp:70-131)   kf = a, kf_b = b; T_prior = T_a_b_prior,
 *                                sqrt_inf 6x6. The factor a pose graph over sparsified windows is made of (SURVEY.md §8f
 *                                rank 2; information from sadvio_ba_marginalize_relative). As coded it composes its deltas on
 *                                the FRAME-TO-WORLD transforms, T_w_a (exp(w), t): in a window that carries such factors the
 *                                kf_T_f_w slots of a and b are read as T_w_a / T_w_b (a pose-graph window passes frame-to-world
 *                                poses; mixing with visual factors, which read the slot as world-to-frame, is the caller's
 *                                business). */
#define SADVIO_SPARSE_RELATIVE_POSE 4
typedef struct sadvio_sparse_prior {
    int32_t type;
    int32_t kf;          /* key-frame index in the window, or -1 */
    int32_t lmk0, lmk1;  /* landmark indices in the window, or -1 */
    double T_prior[12];  /* IMUPriordx; Relative6DPose: T_a_b_prior */
    double v_prior[3], ba_prior[3], bg_prior[3];
    double delta[3];
    double sqrt_inf[225];
    int32_t kf_b;        /* Relative6DPose: the second key-frame */
    int32_t pad;
} sadvio_sparse_prior;

/* Solver options. sadvio_ba_default_options() fills the reference's hard-coded values
 * (AOptimizer.cpp:315-323) and, for everything the reference leaves unset, the defaults of
 * Ceres Solver 2.2.0 (docker/Dockerfile:50), the version the reference pins. */
typedef struct sadvio_solve_options {
    int32_t max_num_iterations;            /* 20 */
    int32_t jacobi_scaling;                /* 1 */
    int32_t max_num_consecutive_invalid_steps; /* 5 */
    int32_t reserved;
    double function_tolerance;             /* 1e-3 */
    double gradient_tolerance;             /* 1e-10 */
    double parameter_tolerance;            /* 1e-8 */
    double initial_trust_region_radius;    /* 1e4 */
    double max_trust_region_radius;        /* 1e16 */
    double min_trust_region_radius;        /* 1e-32 */
    double min_lm_diagonal;                /* 1e-6 */
    double max_lm_diagonal;                /* 1e32 */
    double min_relative_decrease;          /* 1e-3 */
    /* ceres::HuberLoss(a) on the visual factors (0 = no loss function, as localMapBA / singleFrameOptimization):
     * landmarkOptimization and singleFrameVIOptimization use a = sqrt(1.345) (AOptimizer.cpp:102,223). Applied
     * the way Ceres' Corrector does for rho'' <= 0: residual and Jacobian scaled by sqrt(rho'), cost = rho / 2. */
    double huber_a;                        /* 0 */
    /* Ceres' max_solver_time_in_seconds (singleFrameVIOptimization sets 0.005, AOptimizer.cpp:254): checked, as in
     * TrustRegionMinimizer::FinalizeIterationAndCheckIfMinimizerCanContinue, after every iteration — the solve ends with
     * NO_CONVERGENCE once the time since its start exceeds the limit. Measured on the device (constant 100 MHz clock) from
     * the first kernel of the solve. 0 (and the reference's localMapBA: Ceres' default 1e6 s) = no limit.
     * Deviations from Ceres: (i) the clock covers DEVICE time only — host-side flattening, the upload of set_windows and the
     * graph launch are outside it, whereas Ceres counts its preprocessor and wall time from Solve(); a cap therefore binds
     * later here; (ii) the limit is IGNORED on a window sharded over several GPUs (the ranks' clocks are not synchronised:
     * a rank-local decision would desynchronise the collective schedule); (iii) with a limit the iteration count depends on
     * timing, so parity runs keep it at 0. */
    double max_solver_time_in_seconds;     /* 0 */
} sadvio_solve_options;

typedef struct sadvio_solve_summary {
    int32_t iterations;             /* step attempts performed (Ceres iteration count, excl. iteration 0) */
    int32_t num_successful_steps;
    int32_t num_unsuccessful_steps;
    int32_t termination;            /* SADVIO_TERM_* */
    double initial_cost;            /* 1/2 sum r^2 over the reduced program at x0 */
    double final_cost;
    double fixed_cost;              /* cost of residual blocks whose parameters are all constant */
    double final_radius;
} sadvio_solve_summary;

/* Number of usable gfx950 devices (0 when none: every compute call then fails). */
int sadvio_ba_device_count(void);

/* Fill `opts` with the reference's options for localMapBA (AOptimizer.cpp:315-323). */
void sadvio_ba_default_options(sadvio_solve_options *opts);

/* Create / destroy a backend instance. Replaces constructing one optimizer object
 * (slamParameters.cpp:263-282). */
int sadvio_ba_create(const sadvio_ba_config *cfg, sadvio_ba_handle **out);
void sadvio_ba_destroy(sadvio_ba_handle *h);

/* Upload `n_windows` independent windows (a batch: independent sub-windows solved
 * concurrently; n_windows = 1 is the reference's case). Replaces addResidualsLocalMap
 * (…Analytic.cpp:197-314). Clears any factors set by earlier set_* calls.
 * On a handle created with SADVIO_CFG_LONG_TRACKS landmarks with more than 64 observations are accepted (long tracks, see
 * sadvio_flat_window); SADVIO_E_INVALID_ARG with its own
 * text for a landmark above SADVIO_MAX_LONG_TRACK_OBS observations or seen from more than SADVIO_MAX_LONG_TRACK_KF key-frames, and
 * "a landmark has more than 64 observations" on a window sharded over several GPUs and on every handle created without the flag. */
int sadvio_ba_set_windows(sadvio_ba_handle *h, int32_t n_windows, const sadvio_flat_window *windows);
/* One layout build per key-frame: between begin_update and commit_update, set_windows and the factor setters that follow it
 * (set_pose_priors, set_imu_factors, set_sparse_priors, set_dense_prior, set_lines) only RECORD their arguments (validated and
 * copied as usual); commit_update builds the device layout once and uploads everything in one staged copy. Without the
 * bracket every setter rebuilds what it changes — set_sparse_priors the whole tiling, because eliminable pose-to-landmark
 * factors become pseudo-observations of their landmarks — which is what addResidualsLocalMap + addMarginalizationResiduals
 * (…Analytic.cpp:197-426) amount to when they are called back to back. Compute calls are refused inside the bracket. */
int sadvio_ba_begin_update(sadvio_ba_handle *h);
int sadvio_ba_commit_update(sadvio_ba_handle *h);
/* The single-window call the adapter of one optimizer instance uses: set_windows(h, 1, window). */
int sadvio_ba_set_window(sadvio_ba_handle *h, const sadvio_flat_window *window);

/* Line landmarks of window `w` (NULL or n_line = 0 clears them). Not supported on a window sharded over several GPUs. */
int sadvio_ba_set_lines(sadvio_ba_handle *h, int32_t w, const sadvio_line_set *lines);
/* Solved 6-vectors of the lines of window `w` ([n_line][6]), applied as T_w_l <- T_w_l (exp(w), t) (AOptimizer.cpp:334-336). */
int sadvio_ba_get_line_deltas(sadvio_ba_handle *h, int32_t w, double *line_delta6);

/* PosePriordx blocks of window `w` (…Analytic.cpp:224-228). */
int sadvio_ba_set_pose_priors(sadvio_ba_handle *h, int32_t w, int32_t n, const sadvio_pose_prior *priors);

/* IMUFactor + IMUBiasFactor blocks of window `w` (AOptimizer.cpp:55-92). */
int sadvio_ba_set_imu_factors(sadvio_ba_handle *h, int32_t w, int32_t n, const sadvio_imu_factor *factors);

/* Dense marginalisation prior of window `w` = MarginalizationFactor (marginalization.hpp:88-218,
 * added by addMarginalizationResiduals, …Analytic.cpp:316-360): r = r0 + J dx, J is
 * n_full x n row-major. `kf_keep` (or -1 in pure VO) is the key-frame whose 15 states occupy
 * columns [kf_col, kf_col+15) (pose6, v3, ba3, bg3); kept landmark `lmk_index[i]` occupies
 * columns [lmk_col[i], lmk_col[i]+3); lmk_col[i] = -1 means "skipped" (marginalization.hpp:138).
 * J == NULL with n_full == SADVIO_PRIOR_RESIDENT attaches THE HANDLE'S PRIOR — the (J, r0) the last sadvio_ba_marginalize
 * (or sadvio_ba_set_prior) left on the device, the way the reference keeps `_marginalization_last` inside the optimizer
 * (AOptimizer.h:88-90): nothing crosses PCIe; `n` is then ignored, `r0` must be NULL, and the caller only names the
 * variables of THIS window that the prior's columns refer to (it owns the id -> index bookkeeping, like the reference's
 * _map_frame_idx / _map_lmk_idx).
 * A kept landmark must not be a long track (more than 64 observations, see sadvio_flat_window): SADVIO_E_INVALID_ARG, and the
 * window keeps the prior it had; a handle created with SADVIO_CFG_LONG_TRACK_PRIORS keeps a long track like any landmark. */
#define SADVIO_PRIOR_RESIDENT (-1)
int sadvio_ba_set_dense_prior(sadvio_ba_handle *h, int32_t w, int32_t n_full, int32_t n,
                              const double *J, const double *r0, int32_t kf_keep, int32_t kf_col,
                              int32_t n_keep, const int32_t *lmk_index, const int32_t *lmk_col);

/* ---- marginalisation of the oldest key-frame into a dense prior (K8) --------------------------------------
 * Replaces BundleAdjustmentCERESAnalytic::marginalize / Marginalization::{computeInformationAndGradient,
 * computeSchurComplement, rankReveallingDecomposition, computeJacobiansAndResiduals}
 * (…Analytic.cpp:431-663, marginalization.cpp:145-265,318-342,516-530) on window `w` as uploaded by set_windows.
 * The selection of marginalised / kept landmarks (preMarginalize, marginalization.cpp:23-143) is object-graph
 * logic and stays with the caller, who passes the two index lists in the reference's order.
 * Column layout (marginalization.cpp:38-113): marginalised = [frame0 pose 6 (+ v, ba, bg 9 if marg_has_imu) |
 * lmk_marg 3 each]; kept = [frame1 15 states if kf_keep >= 0 | lmk_keep 3 each]. */
/* Eigenvalue cut of the pseudo-inverse of Amm and of the rank-revealing decomposition of Ak.
 *   SADVIO_EIG_CUT_REFERENCE   (0, the default of a zero-initialised request): the reference's arithmetic — keep
 *       lambda > 1e-12, ABSOLUTE (Marginalization::_eps, marginalization.hpp:58, applied at marginalization.cpp:237,322).
 *       In float64 that constant sits below the rounding noise of the sums it is applied to (|A| ~ 1e5..1e8 => noise
 *       ~ 1e-11..1e-8): exactly-null directions are kept or dropped by the sign of a rounding error, in the reference as here;
 *       the prior's INFORMATION (J^T J, J^T r0) is unaffected to rounding (a kept noise direction carries ~1e-11 of it),
 *       only n_full varies. Weakly observed directions (far, low-parallax depth: 1e-12 < lambda < n eps lambda_max) are
 *       KEPT, as the reference keeps them.
 *   SADVIO_EIG_CUT_NOISE_FLOOR (1): keep lambda > max(1e-12, n eps lambda_max) — the numerically meaningful rank; n_full
 *       is reproducible across implementations, at the price of dropping directions whose information is below the floor
 *       (what it drops from Ak itself is <= n eps lambda_max by construction; a direction v dropped from Amm^+ leaves
 *       (Arm v)(Arm v)^T / lambda in Ak. tests/test_gpu_margloop.py measures both modes on a low-parallax window — 300
 *       directions between the cuts: |Ak_ref - Ak_floor|_2 = 2e-10 lambda_max — and bounds the effect on the next solve).
 * Form of the prior handed back / kept on the device (both give the same MarginalizationFactor cost, gradient and
 * Gauss-Newton matrix: r0 + J dx enters the solve only through J^T J, J^T r0 and |r0|^2):
 *   SADVIO_PRIOR_FORM_EIGEN    (0): the reference's J = Lambda^1/2 U^T, r0 = -Lambda^-1/2 U^T bk, rows in ascending
 *       eigenvalue order (marginalization.cpp:318-342,516-530) — one-sided block Jacobi on the device, ~20 ms at n ~ 900.
 *   SADVIO_PRIOR_FORM_CHOLESKY (1): J = G, a Cholesky factor G^T G = Ak, r0 = -G^-T bk by carrying bk through the
 *       factorisation — no eigen-decomposition; sadvio_ba_sparsify then takes Sigma_k = Ak^-1 from the triangular inverse of
 *       G. Two routes (~1 ms / ~2 ms at n ~ 900): under SADVIO_EIG_CUT_REFERENCE with an earlier prior folded in (Ak is then
 *       normally of full rank) the factorisation is UNPIVOTED — G = L^T, upper triangular in the caller's column order,
 *       n_full = n — and every pivot is tested afterwards (positive, above the cut, above the rounding noise of its own
 *       elimination); a failed test, a first marginalisation and SADVIO_EIG_CUT_NOISE_FLOOR (whose point is a reliable
 *       numerical rank, which an unpivoted factorisation cannot give) take the rank-revealing route: diagonal pivoting with
 *       the cut applied to the pivots, G's rows in pivot order. Either way only J^T J, J^T r0 and |r0|^2 are defined by the
 *       form; the rows themselves are not the reference's. */
#define SADVIO_EIG_CUT_REFERENCE 0
#define SADVIO_EIG_CUT_NOISE_FLOOR 1
#define SADVIO_PRIOR_FORM_EIGEN 0
#define SADVIO_PRIOR_FORM_CHOLESKY 1

typedef struct sadvio_marg_request {
    int32_t kf_marg;                 /* frame0 */
    int32_t kf_keep;                 /* frame1 when it carries an IMU (15 columns), else -1 */
    int32_t marg_has_imu;            /* frame0->getIMU() */
    int32_t n_marg;
    const int32_t *lmk_marg;         /* window landmark indices, order of _lmk_to_marg */
    int32_t n_keep;
    const int32_t *lmk_keep;         /* order of _lmk_to_keep */
    const sadvio_imu_factor *imu;    /* IMUFactor + IMUBiasFactor(frame0, frame1) or NULL (…Analytic.cpp:451-508) */
    int32_t n_prior;                 /* PosePriordx blocks (<= 4), .kf = kf_marg or kf_keep (:605-617) */
    const sadvio_pose_prior *priors;
    int32_t last_n_full, last_n;     /* previous MarginalizationFactor (:574-603); last_n_full = 0 if none;
                                        last_n_full = SADVIO_PRIOR_RESIDENT: the handle's prior (last_J / last_r0 / last_n ignored) */
    const double *last_J, *last_r0;
    int32_t last_kf, last_kf_col;    /* window index of its kept frame (= kf_marg now) or -1, its first column */
    int32_t last_n_keep;
    const int32_t *last_lmk_index;   /* window landmark indices of its kept landmarks */
    const int32_t *last_lmk_col;     /* their columns (-1 = skipped) */
    int32_t eig_cut_mode;            /* SADVIO_EIG_CUT_* */
    int32_t prior_form;              /* SADVIO_PRIOR_FORM_* */
} sadvio_marg_request;

typedef struct sadvio_marg_result {
    int32_t m, n, n_full;
    int32_t kf_col;   /* column of kf_keep's 15 states in the new prior, -1 if none */
    int32_t sweeps_mm, sweeps_k;  /* Jacobi sweeps of the two eigen-decompositions (sweeps_k = 0 in the Cholesky form) */
} sadvio_marg_result;

/* Returns SADVIO_E_REFUSED when n < 4 (marginalization.cpp:215-216; the reference then clears its prior, and so does the
 * handle). Outputs (caller-allocated): lmk_col[n_keep] column of each kept landmark in the new prior.
 * The new prior STAYS ON THE DEVICE as the handle's prior (AOptimizer.h:88-90: `_marginalization_last`), replacing the
 * previous one: the next window attaches it with sadvio_ba_set_dense_prior(.., SADVIO_PRIOR_RESIDENT, ..) or sparsifies it
 * with sadvio_ba_sparsify(.., J = NULL, ..), the next marginalisation folds it in with last_n_full = SADVIO_PRIOR_RESIDENT.
 * J / r0 may be NULL (the default path: no read-back); when given, J[n*n] receives the n_full x n prior Jacobian
 * (row-major, packed) and r0[n] the n_full prior residuals.
 * ASYNCHRONOUS without a read-back: the call returns once the host has taken its route decisions; the tail kernels (packing of the
 * prior, the swap into the handle) are stream work like everything that reads the prior afterwards (all on the handle's one stream,
 * so the order is kept). A device fault in that tail therefore surfaces in the NEXT call of this handle that waits (solve,
 * get_deltas, a read-back); SADVIO_DEBUG != 0 or cfg.profile_kernels make marginalize wait itself so that it is attributed here. A
 * consumer on ANOTHER stream or handle must synchronise with this handle first (sadvio_ba_get_prior does).
 * Refused (SADVIO_E_INVALID_ARG) on a window sharded over several GPUs: each rank holds a landmark partition only. */
int sadvio_ba_marginalize(sadvio_ba_handle *h, int32_t w, const sadvio_marg_request *rq, sadvio_marg_result *res,
                          int32_t *lmk_col, double *J, double *r0);

/* Route counters of the Cholesky-form marginalisations of this handle since its creation: calls, calls that took the unpivoted
 * wide-panel factorisation (Ak of full rank, every pivot tested), calls that tried it and fell back to the rank-revealing (pivoted)
 * route. calls - unpivoted - fell_back = calls that pivoted without a try (no earlier prior, or the noise-floor cut). */
int sadvio_ba_marg_stats(sadvio_ba_handle *h, int32_t *calls, int32_t *unpivoted, int32_t *fell_back);

/* Whether the last sadvio_ba_solve of this handle ran the single-round instantiations of its tile kernels: 1 or 0 in
 * *taken. They serve submissions whose every tile holds one landmark round per wave and that need neither the robust loss, a prior
 * that keeps landmarks, nor IMU workgroups; SADVIO_NO_ONE_ROUND=1 (read when the handle is created) keeps the looping kernels. The
 * arithmetic is the same either way. */
int sadvio_ba_one_round(sadvio_ba_handle *h, int32_t *taken);

/* The handle's prior: read-back on request (any pointer may be NULL; J has room for n_full * n, r0 for n_full doubles),
 * upload of a prior kept elsewhere (e.g. restored from a dump; n_full = 0 clears it), and its shape. */
typedef struct sadvio_prior_info {
    int32_t valid, n_full, n, form;
} sadvio_prior_info;
int sadvio_ba_get_prior(sadvio_ba_handle *h, sadvio_prior_info *info, double *J, double *r0);
int sadvio_ba_set_prior(sadvio_ba_handle *h, int32_t n_full, int32_t n, int32_t form, const double *J, const double *r0);

/* NFR sparsification of a dense prior (Marginalization::sparsifyVIO / sparsifyVO, marginalization.cpp:362-514) into
 * the factor list of the sparse branch of addMarginalizationResiduals (…Analytic.cpp:363-426): vio != 0 -> one
 * IMUPriordx on kf_keep + one PoseToLandmarkFactor per kept landmark; vio == 0 -> greedy landmark chain ordered by
 * |tr Lambda_ij|, a Landmark3DPrior on the minimum-entropy landmark + LandmarkToLandmarkFactor links. The prior is
 * the (J, column map) pair produced by sadvio_ba_marginalize / passed to sadvio_ba_set_dense_prior; J == NULL = the
 * handle's prior (n_full / n are then taken from it and the arguments ignored; nothing is uploaded). A host J must be in
 * the EIGEN form (orthogonal rows); the handle's prior may be in either form. Linearisation values (T_f_w, v, ba, bg,
 * landmark positions) are those of window `w`. `out` has room for n_keep + 1 factors. Refused on a sharded window. */
int sadvio_ba_sparsify(sadvio_ba_handle *h, int32_t w, int32_t vio, int32_t n_full, int32_t n, const double *J,
                       int32_t kf_keep, int32_t kf_col, int32_t n_keep, const int32_t *lmk_index, const int32_t *lmk_col,
                       int32_t *n_out, sadvio_sparse_prior *out);

/* ---- relative-pose information between two key-frames (NFR), SURVEY.md §8f rank 2 --------------------------------
 * Replaces BundleAdjustmentCERESAnalytic::marginalizeRelative (…Analytic.cpp:665-809) with
 * Marginalization::preMarginalizeRelative (marginalization.cpp:532-588) on window `w`: every landmark of kf_a that also
 * has a feature in kf_b is marginalised (reprojection factors of its features in the two frames), the two poses are
 * kept (n = 12), Ak -> Sigma_k = pseudo-inverse through the rank-revealing decomposition, and the information of a
 * Relative6DPose(T_w_a, T_w_b, T_a_b = T_a_w T_w_b, sqrt_inf = I) factor is recovered: inf = (J Sigma_k J^T)^-1.
 * As coded: a landmark enters the list once PER feature it has in kf_b, and its factors are added once per entry (stereo
 * landmarks count twice). Frames with IMU states are refused (the reference indexes their velocity / bias columns
 * outside of its own layout, :705-737). Returns SADVIO_E_REFUSED when no landmark is shared, SADVIO_E_INVALID_ARG on a
 * window sharded over several GPUs (each rank only holds its landmark partition: the sum would be partial).
 * Eigenvalue cuts (`eig_cut_mode`, SADVIO_EIG_CUT_* above): REFERENCE drops eigenvalues <= 1e-12 absolutely
 * (Marginalization::_eps) on the 3m x 3m landmark block and on Ak; NOISE_FLOOR uses max(1e-12, m eps lambda_max) on the
 * landmark block and max(1e-12, 12 eps lambda_max (2 + n_items)) on Ak (in float64 the absolute cut sits
 * below the rounding noise of the sums it is applied to — on the reference's own test fixture the null eigenvalue computes
 * to +-1e-11, and the gauge null space of a summed Schur complement to 1e-7 .. 4e-6). With thousands of shared landmarks
 * that floor reaches 1e-8 .. 1e-6 relative to lambda_max ~ 1e7..1e9: directions whose information is below it (far,
 * low-parallax depth) are treated as unobserved, where the reference mode inverts them (and, for an exactly-null
 * direction, inverts its rounding noise: the recovered information is then only meaningful if the pair is well posed).
 * inf36: 6x6 row-major (rotation 3 | translation 3); Ak144 (may be NULL): the 12x12 reduced information. */
int sadvio_ba_marginalize_relative(sadvio_ba_handle *h, int32_t w, int32_t kf_a, int32_t kf_b, int32_t eig_cut_mode, double *inf36,
                                   double *Ak144);

/* The same for n_pair pairs of window `w` in ONE call: what a caller who turns a window into a pose graph asks for (every pair
 * (k, k + 1), (k, k + 2) of a 500-key-frame window is ~1 000 factors). Pair i gives exactly what
 * sadvio_ba_marginalize_relative(h, w, kf_a[i], kf_b[i], eig_cut_mode, ...) defines — the same landmark selection with its
 * multiplicities, the same cuts, the same Sigma_k, J and inverse — computed by one kernel launch (one workgroup per pair, down to
 * the 6 x 6 inverse) behind one host wait, with no device allocation per pair. Deterministic: every sum is taken in a fixed order
 * (no floating-point atomics), two calls return the same bits, and a pair's bits depend neither on the other pairs of the batch
 * nor on its position in it. Duplicate pairs are allowed.
 * status[i] = SADVIO_OK, or SADVIO_E_REFUSED for a pair that shares no landmark or whose 6 x 6 covariance cannot be inverted (a
 * pivot that is exactly zero or not finite); a refused pair has zeros in all its outputs and the call still returns SADVIO_OK.
 * n_pair = 0 returns SADVIO_OK and touches nothing. Argument errors fail the whole call with nothing written, codes as for the
 * single pair: SADVIO_E_INVALID_ARG for a null required pointer, an index out of range, kf_a[i] == kf_b[i], a bad eig_cut_mode, a
 * window with IMU states, a sharded window; SADVIO_E_STATE before set_windows or between begin_update and commit_update.
 * The solve's deltas, summaries and trace and the handle's prior are left untouched. */
int sadvio_ba_marginalize_relative_batch(sadvio_ba_handle *h, int32_t w, int32_t n_pair,
        const int32_t *kf_a, const int32_t *kf_b,   /* [n_pair] */
        int32_t eig_cut_mode,                       /* SADVIO_EIG_CUT_* */
        double *inf36,       /* [n_pair][36], required */
        double *Ak144,       /* [n_pair][144] or NULL */
        double *T_a_b,       /* [n_pair][12] or NULL: T_a_w T_w_b (R row-major 9 | t 3), the T_prior of the Relative6DPose factor */
        int32_t *n_shared,   /* [n_pair] or NULL: landmarks the pair shares (distinct; m = 3 * sum of multiplicities is NOT this) */
        int32_t *status);    /* [n_pair], required: SADVIO_OK | SADVIO_E_REFUSED */

/* ---- one window spanning several GPUs (no reference counterpart: the reference is one process) ----
 * The landmarks of a window (with all their observations) are partitioned over `world` processes, one GPU each;
 * key-frames, cameras, pose priors and IMU factors are replicated. A marginalisation prior rides a sharded window in its
 * SPARSIFIED form (sadvio_ba_sparsify): the IMUPriordx factor is replicated (every rank passes it), each
 * PoseToLandmarkFactor goes to the rank that owns its landmark, with the landmark index of that rank's window — or as the DENSE
 * prior (sadvio_ba_set_dense_prior with host J / r0; round 5): every rank passes the whole prior and carries ALL of its kept landmarks
 * as variables of its window, with their observations on rank 0 only (the others list them without observations;
 * sadvio_amd/sharding.py builds such shards); rank 0 adds J^T J / J^T r to the all-reduced system, every rank evaluates the prior's
 * cost from row-block partials summed in index order (same bits on every rank). HARD PRECONDITION, checked on ranks != 0: a kept
 * landmark has observations on rank 0 only (SADVIO_E_INVALID_ARG otherwise — they would be counted twice in the all-reduced system). Factors that hold landmarks in the reduced system
 * without a dense prior (Landmark3DPrior, landmark chains), the handle-resident prior (SADVIO_PRIOR_RESIDENT: marginalize is not
 * available on a sharded window), line landmarks and marginalize_relative are refused on a sharded window. Every rank calls set_windows with ITS landmarks, then solve(); per LM step the library all-reduces [S | g | diag | per-rank cost partials] once and the
 * step's candidate-cost partials once; every rank then solves the identical reduced system redundantly
 * (no broadcast) and back-substitutes its own landmarks. Pose deltas and summaries are identical on all ranks.
 *
 * set_collective installs a caller-provided in-place sum all-reduce over device memory, enqueued on
 * `hip_stream` (returns 0 on success); comm_init_rccl installs the built-in one (ncclAllReduce, ncclDouble,
 * ncclSum over RCCL / xGMI) from a 128-byte ncclUniqueId created by rank 0 with rccl_unique_id and
 * distributed by the caller. Both must be called before set_windows. */
typedef int (*sadvio_allreduce_fn)(void *ctx, double *device_buf, int64_t count, void *hip_stream);
int sadvio_ba_set_collective(sadvio_ba_handle *h, int32_t rank, int32_t world, sadvio_allreduce_fn fn, void *ctx);
#define SADVIO_RCCL_ID_BYTES 128
int sadvio_ba_rccl_unique_id(void *id128);
int sadvio_ba_comm_init_rccl(sadvio_ba_handle *h, int32_t rank, int32_t world, const void *id128);
/* What the handle's collective really spans: with the built-in RCCL collective the numbers come from the communicator itself
 * (ncclCommCount / ncclCommUserRank / ncclCommCuDevice), otherwise from set_collective. Any pointer may be NULL. */
int sadvio_ba_comm_info(sadvio_ba_handle *h, int32_t *nranks, int32_t *rank, int32_t *device, int32_t *is_rccl);

/* Sparse (NFR) prior factors of window `w`; replaces the previous list (n = 0 clears it). A factor that touches a long track
 * (a landmark with more than 64 observations, see sadvio_flat_window), or pose-to-landmark factors whose two pseudo-observations
 * each would take a landmark past 64, are refused with SADVIO_E_INVALID_ARG; the window keeps the list it had. On a handle created
 * with SADVIO_CFG_LONG_TRACK_PRIORS a factor may touch a long track: it holds the landmark in the reduced system, a pose-to-landmark
 * factor included (see sadvio_flat_window, "Long tracks under a prior"); the second refusal stays. */
int sadvio_ba_set_sparse_priors(sadvio_ba_handle *h, int32_t w, int32_t n, const sadvio_sparse_prior *factors);

/* Run the Levenberg-Marquardt solve of every uploaded window: replaces the body of
 * AOptimizer::localMapBA / localMapVIOptimization from ceres::Solve on (AOptimizer.cpp:326,388).
 * `summaries` has n_windows entries (may be NULL). */
int sadvio_ba_solve(sadvio_ba_handle *h, const sadvio_solve_options *opts, sadvio_solve_summary *summaries);

/* Read back the solved deltas of window `w`; arrays are index-aligned with the window's input
 * arrays (landmark / key-frame order is never permuted). Any pointer may be NULL.
 * The adapter applies them as AOptimizer.cpp:329-340 (poses, landmarks) and :391-418 (v, ba, bg). */
int sadvio_ba_get_deltas(sadvio_ba_handle *h, int32_t w, double *pose_delta6, double *lmk_delta3,
                         double *dv3, double *dba3, double *dbg3);

/* Per-iteration log of the last solve of window `w`: what ceres::Solver::Summary::iterations holds for the reference
 * (AOptimizer.cpp:325-327 keeps the summary; FullReport prints it). Row i (8 doubles) = the state after i step attempts:
 *   [0] cost  [1] cost_change  [2] trust_region_radius  [3] step_norm  [4] relative_decrease  [5] step_is_successful
 *   [6] gradient_max_norm at that state (-1 for the state after the last attempt, which is not linearised again)
 *   [7] model_cost_change of the attempt.
 * Row 0 is the starting point. `n_rows` receives iterations + 1; at most `cap_rows` rows are written. */
int sadvio_ba_get_trace(sadvio_ba_handle *h, int32_t w, int32_t cap_rows, double *rows8, int32_t *n_rows);

/* Echo of the opaque ids of window `w` in output order (bit-exact identity check). */
int sadvio_ba_get_ids(sadvio_ba_handle *h, int32_t w, int64_t *kf_id, int64_t *lmk_id);

/* Linearise window `w` at zero deltas and return per-observation residuals/Jacobians
 * (row-major r[2], J_pose[2x6], J_lmk[2x3]): the GPU counterpart of calling
 * CostFunction::Evaluate on every block (…Analytic.h:52-90 / …Angular….h:55-111). Parity probe. */
int sadvio_ba_linearize(sadvio_ba_handle *h, int32_t w, const double *pose_delta6, const double *lmk_delta3,
                        double *r2, double *J_pose12, double *J_lmk6);

/* ALandmark::sanityCheck / avgChi2err / chi2err (ALandmark.cpp:98-146) for every landmark of window `w`, the gate
 * AOptimizer::landmarkOptimization applies before it writes a landmark back (AOptimizer.cpp:124-141):
 *   avg_chi2[l] = mean over the landmark's observations of |proj - meas|^2 / sigma^2, where an observation whose
 *                 projection fails the tests of Camera::project (depth < 0.1, pixel outside [0,width]x[0,height],
 *                 non-finite; Camera.cpp:26-52) counts 1000;
 *   inlier[l]   = (n_obs >= 2 && avg_chi2 <= 2)   (95 % chi2 test on a 2-D detection).
 * `image_wh` = n_cam x (width, height) of the caller's cameras (NULL: (2 cx, 2 cy), the bound the factors use).
 * Evaluated at the deltas given (NULL = zeros = the linearisation origin; the reference tests the landmark's pose
 * BEFORE the solved delta is applied). sigma is the FEATURE's pixel sigma (AFeature::getSigma, 1.0 everywhere in the
 * reference, AFeature2D.h:18): `pixel_sigma` > 0 sets it; <= 0 selects the window's cam_sigma for pixel windows and
 * 1.0 for angular windows (whose cam_sigma is an angle). Angular windows: the measured pixel is recovered from the
 * stored bearing through K. Either output may be NULL. */
int sadvio_ba_landmark_chi2(sadvio_ba_handle *h, int32_t w, const double *pose_delta6, const double *lmk_delta3,
                            const double *image_wh, double pixel_sigma, double *avg_chi2, int32_t *inlier);

/* The same gate for rigs whose cameras are not pinholes: every observation is projected by its camera's OWN model,
 * as ALandmark::chi2err does through ImageSensor::project (Camera.cpp:26-52, fisheye.cpp:127-172, 195-240,
 * DoubleSphere.cpp:33-78; restated on the host by project_camera of sadvio_cameras.hpp, which the device follows line
 * for line). `models` = one entry per camera of window `w` in the caller's camera order; fx fy cx cy are the window's
 * cam_K. Validity tests (a failed projection counts 1000): pinhole z < 0.1; the three fisheye laws z < 0.01; omni and
 * double sphere return early with u = v = 0 when z < 0.1 and test the cone z <= -w d (w from alpha <= 0.5 or > 0.5);
 * all models test [0,width]x[0,height] and finiteness. Omni applies p + distort(p) once when `distortion` is set.
 *
 * Measured pixel: `obs_uv` ([n_obs][2], the caller's observation order of the window) is used as it stands on both
 * factor types (the reference compares with the feature's pixel). NULL: a pixel window uses obs_meas; an angular window
 * uses the model's projection of the stored bearing with no validity test applied to it (a pinhole: K b / b_z + c, the
 * expression of sadvio_ba_landmark_chi2). CAVEAT: Fisheye's ray is 0/0 at the principal point (Fisheye::getRayCamera
 * divides by the radius), so the bearing stored for such a feature carries no pixel: a caller with features at the
 * principal point of a fisheye camera passes `obs_uv`.
 *
 * Everything else is sadvio_ba_landmark_chi2: deltas (NULL = zeros), `pixel_sigma`, inlier = (n_obs >= 2 && !(avg > 2)),
 * pseudo-observations of sparse prior factors are skipped. `obs_chi2` ([n_obs], caller's order, or NULL) receives each
 * observation's term of the sum (1000 for a failed projection). A table of pinholes gives avg_chi2 the bits of
 * sadvio_ba_landmark_chi2 with image_wh = the models' (width, height).
 * Errors: SADVIO_E_STATE before set_windows or between begin_update and commit_update; SADVIO_E_INVALID_ARG for a null
 * `models`, an unknown kind, a window out of range, or two cameras that the handle stores once (same K, T_s_f, sigma)
 * whose models or image sizes differ (all fields are compared). The solve's deltas, summaries, trace and the handle's
 * prior are untouched; outputs are written on success only. */
#define SADVIO_CAM_PINHOLE 0
#define SADVIO_CAM_FISHEYE_EQUIDISTANT 1
#define SADVIO_CAM_FISHEYE_EQUISOLID 2
#define SADVIO_CAM_FISHEYE_STEREOGRAPHIC 3
#define SADVIO_CAM_OMNI 4
#define SADVIO_CAM_DOUBLE_SPHERE 5
typedef struct sadvio_camera_model {
    int32_t kind;         /* SADVIO_CAM_* */
    int32_t distortion;   /* Omni only: 1 = apply D */
    double width, height; /* image bounds (the image_wh of sadvio_ba_landmark_chi2) */
    double rmax;          /* Fisheye::_rmax */
    double xi, alpha;     /* Omni / DoubleSphere */
    double D[4];          /* k1 k2 p1 p2 */
} sadvio_camera_model;

int sadvio_ba_landmark_chi2_models(sadvio_ba_handle *h, int32_t w, const double *pose_delta6, const double *lmk_delta3,
                                   const sadvio_camera_model *models, const double *obs_uv, double pixel_sigma,
                                   double *avg_chi2, int32_t *inlier, double *obs_chi2);

/* ---- visual-inertial initialisation: AOptimizer::VIInit (AOptimizer.cpp:448-581) ----
 * Unknowns: the gravity direction r_wi (2 parameters, R_w_i = exp_so3((r0, r1, 0)), :464-466, :537), one velocity
 * delta per frame that an IMUFactorInit touches (:459-463), the log-scale lambda (:478-481; constant unless
 * optim_scale) and the bias deltas dba, dbg (constant in VIInit, :469-476; `optim_bias` frees them, which is how the
 * reference's own factor test drives IMUFactorInit, imu_test.cpp:505-545). Residuals: IMUFactorInit
 * (residuals.hpp:302-410) per pair, + the two bias priors Landmark3DPrior(0, 0, I / sigma) (:503-516) when the biases
 * are free. Solved with the same Ceres-2.2 LM rules as the window solves (the reference: 50 iterations, f_tol 1e-3). */
typedef struct sadvio_viinit_problem {
    int32_t n_frames;
    int32_t n_factors;
    const double *T_f_w;              /* [n_frames][12] */
    const double *vel;                /* [n_frames][3] IMU::getVelocity of each frame */
    const sadvio_imu_factor *factors; /* IMUFactorInit(imu_i, imu_j): kf_i / kf_j index the frames (pairing rule :485-500:
                                         i = imu_j->getLastKF(), i != j); dt, delta_*, J_*, cov are read */
    int32_t optim_scale;
    int32_t optim_bias;
    double sigma_dba, sigma_dbg;      /* sqrt(dt_window) * b{acc,gyr}_noise (:504-512); read only when optim_bias */
} sadvio_viinit_problem;

typedef struct sadvio_viinit_result {
    double r_wi[2];
    double lambda;
    double dba[3], dbg[3];
    double R_w_i[9]; /* exp_so3((r_wi, 0)) row-major: what VIInit hands back through its R_w_i argument */
    double scale;    /* exp(lambda): VIInit's return value (:575) */
} sadvio_viinit_result;

/* dv3: [n_frames][3] velocity deltas (zero for frames no factor touches). The adapter applies the result as
 * AOptimizer.cpp:526-562 (velocities, T_f_w.translation() *= scale, T_f_w = T_f_w * T_w_i, landmarks, priors).
 * At most 48 frames (the whole solve runs inside one workgroup). */
int sadvio_ba_vi_init(sadvio_ba_handle *h, const sadvio_viinit_problem *prob, const sadvio_solve_options *opts,
                      sadvio_solve_summary *summary, sadvio_viinit_result *res, double *dv3);

/* ---- metric scale of a non-overlapping rig: AngularAdjustmentCERESAnalytic::landmarkOptimizationNoFov
 *      (AngularAdjustmentCERESAnalytic.cpp:741-907, declared virtual in AOptimizer.h:34) ----
 * Unknowns: the scale lambda of T_cam0_cam0p's translation (a plain value starting at 1.0, :755-757) and one additive delta
 * per landmark (:802-804); every pose is constant (:760-762, :836-841). Residuals per landmark, all under
 * HuberLoss(opts->huber_a) (:753): AngularErrorScaleCam0 on fp's feature (…Analytic.h:122-194, weight 1 / sigma^2,
 * sigma = 1, :806-817) and AngularErrCeres_pointxd_dx on f's feature and on every other key-frame's feature (:819-849,
 * sigma = 1); plus scalePrior(info_scale) on lambda (residuals.hpp:702-717, no loss, :853-854). LM with the Ceres-2.2 rules
 * of the window solves (:857-868: 20 iterations, f_tol 1e-3); Ceres' x_norm includes lambda's value. The landmark selection
 * (:775-851) is the caller's: see nofov_flatten in sadvio_optimizer.hpp. */
typedef struct sadvio_nofov_problem {
    int32_t n_lmk;                /* landmarks with both feat and featp (:820) */
    int32_t n_obs;                /* fixed-pose angular factors, all landmarks */
    int32_t n_frames;             /* key-frames the factors read; frame 0 is f */
    int32_t n_cam;
    int32_t cam0;                 /* f's sensor 0 (:767): index into cam_T_s_f */
    int32_t fix_scale;            /* -1: the reference's rule, |log_so3(R)| < 0.05 or |t| < 0.01 (:769-772); 0 / 1: force */
    const double *frame_T_f_w;    /* [n_frames][12] getWorld2FrameTransform (:827, :845); T_cam0_w = T_s_f[cam0] * T_f_w[0] (:813) */
    const double *cam_T_s_f;      /* [n_cam][12] getFrame2SensorTransform (:809-810, :826, :844) */
    const double *T_cam0_cam0p;   /* [12] the motion whose translation is scaled (:814) */
    double info_scale;            /* scalePrior's sqrt information (:853) */
    double gate;                  /* 2 / focal of f's sensor 0 (:890, Camera.h:46) */
    const double *lmk_p;          /* [n_lmk][3] lmk->getPose().translation() (:812) */
    const double *scale_bearing;  /* [n_lmk][3] featp's bearing (:811) */
    const int32_t *scale_cam;     /* [n_lmk] featp's sensor: T_cam_cam0 = T_s_f[scale_cam] * T_s_f[cam0]^-1 (:808-810) */
    const int32_t *lmk_obs_ptr;   /* [n_lmk + 1] CSR of the fixed-pose angular factors of each landmark (f's first, then feats) */
    const int32_t *obs_frame;     /* [n_obs] frame of the factor's feature */
    const int32_t *obs_cam;       /* [n_obs] sensor of the factor's feature: index into cam_T_s_f */
    const double *obs_bearing;    /* [n_obs][3] getBearingVectors().at(0) (:826, :843) */
} sadvio_nofov_problem;

typedef struct sadvio_nofov_result {
    double lambda;       /* the solved scale (:872) */
    int32_t usable;      /* IsSolutionUsable && 0.5 <= lambda <= 1.5 (:870-871) */
    int32_t scale_fixed; /* lambda was held constant (:769-772) */
    int32_t n_inliers;   /* landmarks that pass the gate (:889-899) */
    int32_t pad;
} sadvio_nofov_result;

/* lmk_delta3: [n_lmk][3] solved deltas; gate_norm: [n_lmk] |r| of the scale factor at the solution without loss (:884-887);
 * inlier: [n_lmk] 1 iff !(gate_norm > gate). Any output may be NULL. Returns SADVIO_E_NOT_USABLE when the solution is not
 * usable or lambda is out of [0.5, 1.5] (the reference then returns false and changes nothing); the outputs are filled anyway.
 * At most 65 536 landmarks and 16 angular factors per landmark (one workgroup solves the whole problem);
 * n_lmk = 0 with lambda constant is SADVIO_E_INVALID_ARG. opts->huber_a applies to the visual factors only. */
int sadvio_ba_nofov_scale(sadvio_ba_handle *h, const sadvio_nofov_problem *prob, const sadvio_solve_options *opts,
                          sadvio_solve_summary *summary, sadvio_nofov_result *res, double *lmk_delta3, double *gate_norm,
                          int32_t *inlier);

/* ---- marginal covariances of a solved window ----
 * No reference counterpart as one call; the quantities the pipeline is written to consume: Sigma_k of the NFR sparsification
 * (marginalization.cpp:259-262), covdT of the ESKF (ESKFEstimator.cpp:180), the 6 x 6 covariance of an odometry message.
 * Evaluated for window `w` after sadvio_ba_solve, at the solve's final accepted state (the linearisation origin composed with the
 * deltas get_deltas returns): H = J^T J over every residual block of the window — Gauss-Newton, no LM damping, no Jacobi scaling;
 * the visual factors under HuberLoss(opts.huber_a) of that solve, corrected as the solve corrects them (ceres::Covariance applies
 * the loss by default) — restricted to the free parameters; Sigma = H^-1, of which only the blocks asked for are formed, by the
 * solve's own elimination: S = H_pp - sum_l H_pl H_ll^-1 H_lp over the eliminated landmarks, Sigma_pp = S^-1 (unpivoted Cholesky,
 * every pivot tested), Sigma_ll = H_ll^-1 + W_l Sigma_pp W_l^T with W_l = H_ll^-1 H_lp.
 * Coordinates: the library's delta coordinates — a key-frame's block is over (w, t) of T_f_w = T_f_w0 * (exp(w), t)
 * (geometry.h:198-203) followed, with has_imu, by v, ba, bg; a landmark's over its additive delta (geometry.h:205-210).
 * sadvio_optimizer.hpp maps a key-frame block to the covariance of T_w_f in the order of a ROS pose message. */
typedef struct sadvio_cov_request {
    int32_t n_kf;
    const int32_t *kf;      /* [n_kf] key-frame indices of the window */
    int32_t n_pair;
    const int32_t *pair_a;  /* [n_pair] cross blocks Sigma(a, b) between two key-frames: rows a, columns b */
    const int32_t *pair_b;  /* [n_pair] */
    int32_t n_lmk;          /* -1: every landmark of the window, in its order (`lmk` is not read) */
    const int32_t *lmk;     /* [n_lmk] landmark indices of the window */
} sadvio_cov_request;

/* kf_cov: [n_kf][d][d], d = 6 (15 with has_imu), row-major, state order pose6 | v3 | ba3 | bg3; pair_cov: [n_pair][d][d];
 * lmk_cov: [n_lmk][9]. A kf_const key-frame or lmk_const landmark has no row or column in H: its blocks are all zeros. A landmark
 * kept in the reduced system (prior-kept, chained) has its block taken from Sigma_pp. A landmark whose H_ll is not positive
 * definite (a single observation; a pivot within 64 ulps of its diagonal entry) is left out of H with its observations, gets nine
 * NaNs and is counted in n_lmk_singular (among the landmarks asked for); the call still returns SADVIO_OK.
 * Any output pointer may be NULL. The call waits for its own results; the solve's deltas, summary, trace and the handle's prior are
 * left untouched (a get_deltas after it returns the same bits as before it), and two calls return the same bits (every sum is
 * taken in a fixed order: no floating-point atomics).
 * Returns SADVIO_E_STATE before a solve or inside a begin_update bracket; SADVIO_E_INVALID_ARG for an index out of range, for a
 * window sharded over several GPUs, a window with line landmarks, or a batch the throughput kernels solved (the error text says
 * which), and for a reduced system of 2047 columns or more that is not bandable (below); SADVIO_E_NOT_USABLE when the factorisation
 * of S meets a pivot that is not safely positive (gauge not fixed: no constant key-frame and no prior) — the outputs are then
 * untouched.
 * The band route. A window without a dense prior, landmarks kept in the reduced system or line landmarks has a block-banded S: no
 * non-zero at |i - j| >= bw = (hb + 1) d, hb the largest distance in free key-frame index that a landmark, an IMU pair or a
 * relative-pose factor of the sparsified prior couples (the rule of the solve's band routes). It is BANDABLE when N_p > 0, bw < N_p
 * and bw + nb <= 128 (nb = 6, or 5 with has_imu: the band route's LDS image; d = 6: hb <= 19, d = 15: hb <= 7). For such a window
 * the band of Sigma_pp follows from the band Cholesky factor by the Takahashi recursion (O(N_p bw^2) work, one workgroup, FP64, the
 * same three pivot tests), pair blocks of key-frames further apart than hb by band substitution, and only the blocks asked for
 * travel to the host. pair(a, b) and pair(b, a)^T are equal to the bit; a pair's bits do not depend on the other pairs asked for.
 * Environment variable SADVIO_COV_BAND, read when the handle is created: unset, a bandable window takes the band route only where
 * the call was refused before (N_p >= 2047), so no window served before changes a bit; 1, every bandable window takes it (tests,
 * A/B timing); 0, never (the 2047-column refusal included). In sadvio_ba_get_kernel_times the route shows as the classes cov_band
 * (forward sweep), cov_band_sel (backward sweep), cov_band_pairs and cov_band_gather in place of cov_invert.
 * The border route: long windows with loop closures. One far coupling (a landmark seen again hundreds of key-frames later, one
 * SADVIO_SPARSE_RELATIVE_POSE factor between distant key-frames) makes hb about the number of free key-frames, and the window is no
 * longer bandable. A CLOSURE EDGE is a coupled pair of free key-frames more than hb_lim apart (hb_lim = 19 at d = 6, 7 at d = 15: the
 * band route's limit); the BORDER is a vertex cover of the closure edges, built greedily (the key-frame that covers the most
 * uncovered edges, the lowest index on a tie). The window is BORDERABLE when it has no dense prior, no landmarks kept in the reduced
 * system and no lines, the border has 0 < m <= 96 columns, and the core (the other free key-frames, natural order, n_b columns, band
 * bw' <= (hb_lim + 1) d by construction) has n_b > bw'. With the columns ordered [core | border], S = [B C; C^T D]: the band of
 * B^-1 comes from the band route's two sweeps on B, W = B^-1 C from band substitution, T = D - C^T W is factored densely with the
 * same three pivot tests (the pivots of B followed by those of T are the pivots of S in this order), and
 *     Sigma_DD = T^-1,  Sigma_BD = -W T^-1,  Sigma_BB(i, j) = B^-1(i, j) + (W T^-1 W^T)(i, j)
 * are formed inside the core's band and on the border's rows and columns, which is every block a landmark block reads. Pair blocks
 * of two core key-frames outside the band come from band substitution on B plus the same correction. pair(a, b) and pair(b, a)^T
 * are equal to the bit, and a pair's bits do not depend on the other blocks asked for. Environment variable SADVIO_COV_BORDER, read
 * when the handle is created: unset, a borderable window takes the route only where the call was refused before (N_p >= 2047 and
 * not bandable), so no window served before changes a bit; 1, every borderable window takes it, in front of the band route (tests,
 * A/B timing); 0, never. SADVIO_COV_BORDER_HB lowers hb_lim (tests). In sadvio_ba_get_kernel_times the route adds the classes
 * cov_border_split, cov_border_solve, cov_border_schur and cov_border_apply to the band route's. sadvio_ba_covariance_cross does
 * not take this route: it keeps refusing a window of 2047 columns or more that is not bandable.
 * The square-root assembly. A landmark millimetres from a camera centre puts 1e12 and more into H_pp beside entries of S of 1e10;
 * S = H_pp - sum_l H_pl H_ll^-1 H_lp then loses its digits to the subtraction (5e-4 of relative error in a key-frame block at 1 mm)
 * and comes out indefinite at 0.1 mm. The second assembly forms the same S and landmark blocks without that difference: per
 * eliminated landmark J_l = Q1 R (Gram-Schmidt with a second orthogonalisation pass), C_a = Q1^T J_p,a per observing free key-frame,
 * the landmark's share of block (a, b) of S as the sum over its rows of A_a^T A_b with A_a = [row is a's] J_p,a - Q1 C_a (the pose rows
 * projected on the complement of range(J_l), then squared), and Sigma_ll = R^-1 (I + C Sigma_pp C^T) R^-T. It stays at the float64
 * floor whatever the landmark's depth, S cannot come out indefinite and Sigma_ll is positive semi-definite by construction. The
 * singular-landmark rule is the one above stated through R (fewer than two observations, or r_ii^2 <= 64 eps |column i of J_l|^2); the
 * other terms of S, the inversion (dense or band route), the pivot tests, the fixed order of every sum and the bit guarantees above are
 * unchanged.
 * Environment variable SADVIO_COV_SQRT, read when the handle is created: unset, the plain assembly runs first, and only when the
 * pivot tests refuse its S (either route) the call assembles again in square-root form, inverts and tests again, and returns
 * SADVIO_E_NOT_USABLE only if that fails too — the outputs stay untouched until a form has passed, no window served before changes a
 * bit, and a window refused before pays one more assembly (and one further wait) before the same refusal; 1, the square-root
 * assembly from the start (any front-end that does not cull landmarks closer than a few centimetres: the plain form's loss is silent
 * before it is refused); 0, never. In sadvio_ba_get_kernel_times the assembly shows as the class cov_assemble_sqrt in place of
 * cov_assemble (after a retry, both).
 * A window with long tracks (see sadvio_flat_window) is refused with SADVIO_E_INVALID_ARG and a text that names them, unless the handle
 * was created with SADVIO_CFG_LONG_TRACK_COVARIANCE: then it is served as any window, its long tracks through two kernels of their
 * own (classes k_cov_long, inside the assembly's span, and k_cov_lmk_long in sadvio_ba_get_kernel_times). */
int sadvio_ba_covariance(sadvio_ba_handle *h, int32_t w, const sadvio_cov_request *rq, double *kf_cov, double *pair_cov,
                         double *lmk_cov, int32_t *n_lmk_singular);

/* ---- marginal covariances of many windows of the solved batch in one call ----
 * Item i is exactly what sadvio_ba_covariance(h, items[i].w, &items[i].rq, kf_cov, pair_cov, lmk_cov, &n_lmk_singular) defines: the
 * same H (Gauss-Newton at the final accepted state, the Huber corrector of the last solve), the same singular-landmark rule (nine
 * NaNs, counted), zeros for constant variables, prior-kept landmarks taken from Sigma_pp, the same coordinates and output shapes. A
 * window may appear in several items; the items of a window share its work on the device.
 * route (out) says how Sigma_pp = S^-1 was formed:
 *   SADVIO_COV_ROUTE_NONE   N_p = 0 (every key-frame constant, nothing kept): Sigma_ll = H_ll^-1. Same bits as the single call.
 *   SADVIO_COV_ROUTE_LDS    0 < N_p <= 176: S is factored, inverted and squared inside one workgroup's LDS, all such items of the
 *                           call in a fixed number of launches behind ONE wait. Another factorisation order than the single
 *                           call's: equal within rounding, not to the bit.
 *   SADVIO_COV_ROUTE_DENSE  N_p > 176: the route of sadvio_ba_covariance, item by item. Same bits as the single call.
 *   SADVIO_COV_ROUTE_BAND   a window that sadvio_ba_covariance sends down its band route (see there and SADVIO_COV_BAND: by default
 *                           a bandable window of 2047 columns or more), item by item through the single call's steps. Same bits as
 *                           the single call.
 *   SADVIO_COV_ROUTE_BORDER a window that sadvio_ba_covariance sends down its border route (see there and SADVIO_COV_BORDER: by
 *                           default a borderable window of 2047 columns or more that is not bandable), item by item through the
 *                           single call's steps. Same bits as the single call.
 * The environment variable SADVIO_COV_BATCH_LDS=0 (read when the handle is created) sends every item with N_p > 0 down the DENSE
 * route. The LDS and NONE items are processed in groups of windows whose work arrays stay under 1 GiB
 * (SADVIO_COV_BATCH_SCRATCH_MB overrides the figure; a window larger than the budget is a group of its own); the grouping does not
 * change a bit of the results.
 * The square-root assembly (sadvio_ba_covariance, SADVIO_COV_SQRT): DENSE and BAND items go through the single call's steps and
 * inherit its choice of assembly and its retry. With SADVIO_COV_SQRT=1 the LDS items are sent down the DENSE route (as
 * SADVIO_COV_BATCH_LDS=0 does) and a NONE item's landmark blocks are R^-1 R^-T. With the variable unset, an LDS item that would get
 * SADVIO_E_NOT_USABLE is first retried on its own through the single call's steps in square-root form (one further wait per such
 * item); the bits of items that were served before do not change.
 * Unlike sadvio_ba_covariance, the call accepts a batch the throughput kernels solved (65 536 landmarks or more).
 * status (out) is SADVIO_OK, or SADVIO_E_NOT_USABLE for an item whose S has a pivot that is not safely positive (not finite, not
 * above 1e-12 / N_p, or below 1024 N_p eps of its diagonal entry of S: gauge not fixed). Such an item's outputs are untouched, the
 * other items are unaffected and the call returns SADVIO_OK.
 * Argument errors fail the whole call before anything is written, in any item, with the single call's codes: SADVIO_E_STATE before
 * a solve or inside a begin_update bracket; SADVIO_E_INVALID_ARG for n_item < 0, null `items` with n_item > 0, an index out of
 * range in any item, a handle sharded over several GPUs, a window with line landmarks, a reduced system of 2047 columns or more
 * that is not bandable.
 * n_item = 0 returns SADVIO_OK and touches nothing.
 * No floating-point atomics: two calls return the same bits, and an item's bits depend neither on the other items of the call nor
 * on its position among them. The solve's deltas, summaries, trace and the handle's prior are left untouched.
 * A window with long tracks is served on a handle created with SADVIO_CFG_LONG_TRACKS | SADVIO_CFG_LONG_TRACK_COVARIANCE |
 * SADVIO_CFG_LONG_TRACK_BATCH, on every route and with every guarantee above: on the LDS and NONE routes a long track's rows of the
 * unit's tables and its landmark block come from one workgroup per track (kernel classes k_covb_long and k_covb_lmk_long, which
 * appear only when a group holds a long track), the other routes are the single call's. On every other handle an item that names
 * such a window fails the whole call (SADVIO_E_INVALID_ARG, a text that names long tracks) before anything is written. */
#define SADVIO_COV_ROUTE_NONE  0
#define SADVIO_COV_ROUTE_LDS   1
#define SADVIO_COV_ROUTE_DENSE 2
#define SADVIO_COV_ROUTE_BAND  3
#define SADVIO_COV_ROUTE_BORDER 4

typedef struct sadvio_cov_batch_item {
    int32_t w;               /* in: window of the batch */
    int32_t status;          /* out: SADVIO_OK | SADVIO_E_NOT_USABLE */
    int32_t n_lmk_singular;  /* out: among the landmarks asked for */
    int32_t route;           /* out: SADVIO_COV_ROUTE_* */
    sadvio_cov_request rq;   /* in: as for sadvio_ba_covariance */
    double *kf_cov;          /* out, caller-allocated, any may be NULL; shapes as for sadvio_ba_covariance */
    double *pair_cov;
    double *lmk_cov;
} sadvio_cov_batch_item;

int sadvio_ba_covariance_batch(sadvio_ba_handle *h, int32_t n_item, sadvio_cov_batch_item *items);

/* ---- key-frame x landmark cross covariances of a solved window, and the innovation gate of candidate observations ----
 * Candidate i names key-frame kf[i] (a) and landmark lmk[i] (l) of window `w`. The call returns the cross block Sigma(a, l) of
 * Sigma = H^-1 and, with a candidate camera and measurement, the innovation covariance of that observation
 *   P = J_a Sigma_aa J_a^T + J_a Sigma_al J_l^T + J_l Sigma_la J_a^T + J_l Sigma_ll J_l^T + I
 * and the squared Mahalanobis distance maha2 = r^T P^-1 r of its residual: the uncertainty-aware counterpart of
 * sadvio_ba_landmark_chi2 (maha2 <= 5.99 gates a match at 95 %, two degrees of freedom).
 * Same H as sadvio_ba_covariance: Gauss-Newton at the final accepted state of the last solve, that solve's Huber corrector on the
 * window's own factors, the same free parameters, singular-landmark rule and delta coordinates; Sigma_al = -sum_e Sigma_pp(a, c_e)
 * W_e^T over the landmark's observing free key-frames, in list order (square-root assembly: -(sum_e Sigma_pp(a, c_e) C_e^T) R^-T).
 * The candidate's own residual r and Jacobians J_a (2 x 6, on the pose part of the key-frame's block: the IMU states contribute
 * nothing), J_l (2 x 3) are the window's factor type (pixel or angular) evaluated at that state with the candidate's camera and
 * measurement, whitened by the camera's cam_sigma — so the noise term of P is I — and carry NO robust loss.
 *   constant key-frame        Sigma_al = 0 and P = J_l Sigma_ll J_l^T + I
 *   constant landmark         Sigma_al = 0 and P = J_a Sigma_aa J_a^T + I
 *   landmark kept in the reduced system   Sigma_al is read from Sigma_pp at the landmark's reduced columns
 *   singular landmark         all three outputs NaN and status SADVIO_CROSS_LMK_SINGULAR (also with a constant key-frame); the
 *                             call still returns SADVIO_OK
 *   pixel window, the projection fails Camera::project's tests (depth below 0.1, outside the image)   status
 *                             SADVIO_CROSS_PROJ_INVALID; r = 0 as in the solve, so maha2 = 0; P is still formed from the Jacobians
 *                             the factor keeps
 * Calling rules as for sadvio_ba_covariance: any output pointer may be NULL; innov_cov or maha2 non-NULL with cam == NULL is
 * SADVIO_E_INVALID_ARG, as are cam without meas and a cam index out of the caller's camera range; n = 0 returns SADVIO_OK and touches
 * nothing. The same refusals with the same error texts: SADVIO_E_STATE before a solve or inside a begin_update bracket;
 * SADVIO_E_INVALID_ARG for an index out of range, a sharded handle, line landmarks, a batch the throughput kernels solved, a
 * reduced system of 2047 columns or more that is not bandable; SADVIO_E_NOT_USABLE with the outputs untouched when the pivot tests
 * refuse S. The call inherits the choice of assembly and the retry (SADVIO_COV_SQRT) and the route (SADVIO_COV_BAND) of
 * sadvio_ba_covariance; on the band route the whole block row Sigma(a, :) of every distinct key-frame asked for is formed by band
 * substitution and EVERY candidate is served from it, so a candidate's bits do not depend on where its observers lie; no entry of
 * Sigma outside the band is read. The call waits once for its results (plus the waits sadvio_ba_covariance itself has).
 * Every sum is taken in a fixed order, no floating-point atomics: two calls return the same bits, a candidate's bits depend neither
 * on the other candidates nor on its position, the output order is the request order and repeats are allowed. The solve's deltas,
 * summaries, trace, the handle's prior and every bit sadvio_ba_covariance / _batch return are left as they are.
 * In sadvio_ba_get_kernel_times the step shows as the class cov_cross, on the band route also cov_band_rows. A block row of more
 * than 16 384 doubles (d = 6: N_p > 2 730; d = 15: N_p > 1 092) is read from global memory instead of LDS; the environment variable
 * SADVIO_COV_CROSS_STAGE (read when the handle is created) lowers that figure (tests).
 * A window with long tracks: refused as by sadvio_ba_covariance, and served on a handle created with
 * SADVIO_CFG_LONG_TRACK_COVARIANCE — a candidate on a long track is a candidate like any other. */
#define SADVIO_CROSS_OK            0
#define SADVIO_CROSS_LMK_SINGULAR  1
#define SADVIO_CROSS_PROJ_INVALID  2

typedef struct sadvio_cov_cross_request {
    int32_t n;            /* candidates */
    const int32_t *kf;    /* [n] key-frame index of window w */
    const int32_t *lmk;   /* [n] landmark index of window w */
    const int32_t *cam;   /* [n] camera of the candidate observation (the caller's camera order, as obs_cam); NULL: cross blocks only */
    const double *meas;   /* [n][2] pixel uv | [n][3] unit bearing, as obs_meas of the window's factor type; NULL iff cam is NULL */
} sadvio_cov_cross_request;

int sadvio_ba_covariance_cross(sadvio_ba_handle *h, int32_t w, const sadvio_cov_cross_request *rq,
                               double *cross_cov,  /* [n][d][3]  Sigma(a, l): rows = the key-frame's d states (6 | 15), columns = the landmark */
                               double *innov_cov,  /* [n][4]     P, row-major 2 x 2, of the WHITENED residual (so the noise term is I) */
                               double *maha2,      /* [n]        r^T P^-1 r */
                               int32_t *status);   /* [n]        SADVIO_CROSS_OK | _LMK_SINGULAR | _PROJ_INVALID */

/* Average device time in microseconds per kernel class since the last set_windows, measured
 * with hipEvents on the handle's stream (cfg.profile_kernels = 1). `names` receives pointers
 * to static strings. Returns the number of classes written (<= cap). */
int sadvio_ba_get_kernel_times(sadvio_ba_handle *h, int32_t cap, const char **names, double *avg_us,
                               int64_t *launches);

/* Text of the last error of handle `h` (owned by the handle; valid until its next failing call or sadvio_ba_destroy).
 * h = NULL: why the calling THREAD's last sadvio_ba_create refused its configuration (SADVIO_E_INVALID_ARG) — the text is kept per
 * thread, is cleared by that thread's next sadvio_ba_create and is valid until then; "null handle" when there is none. */
const char *sadvio_ba_last_error(sadvio_ba_handle *h);
const char *sadvio_ba_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SADVIO_BA_H */
