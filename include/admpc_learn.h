/*
 * admpc_learn.h -- fitting the residual GP of a handle on the device from the steps a fleet has taken: observe -> bin -> fit -> install
 * (libadmpc.so; csrc/admpc_learn.hip).  An addition to admpc.h, admpc_fleet.h, admpc_lane.h and admpc_plant.h, whose conventions hold
 * here: device pointers owned by the caller, `stream` a hipStream_t passed as void*, 0 or a negative ADMPC_E* code returned,
 * admpc_last_error() for the message, the caller's HIP device restored, no host synchronisation and no allocation, every refusal in
 * front of the first device call.
 *
 * Scope: the hyperparameters of every regressor (length scales, sigma_f, noise) are GIVEN.  The reference searches them with L-BFGS over
 * the marginal likelihood (model_fitting/gp.py:302-320, DESIGN section 8: GP fitting); that search is not part of this library.  (A grid
 * search of the same likelihood on the device, which feeds the install below, is in admpc_hyper.h.)  What is fitted here is the weight vector alpha = K^-1 (t - ymean) and ymean of a squared-exponential GP at fixed hyperparameters, over at most
 * ADMPC_GP_MAX_POINTS points, each the mean of the samples that fell into one bin of a regular grid over the features.  The quadrotor
 * learns through admpc_quad_learn.h, which takes AdmpcGpBins from here and shares the bodies of the bin kernel and of the fit
 * (csrc/gp_fit_dev.h); the entries below serve the car.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/...)                                replaced by
 *   ----------------------------------------------------------------------------------  ------------------------------------
 *   src/model_fitting/gp_common.py:88-91    y_err = (x_out - x_pred) / dt of a step       admpc_observe_batch: samples
 *   src/model_fitting/gp_common.py:101-112  prune_dataset: the data set cut into bins     admpc_observe_batch: bins
 *   src/model_fitting/gp.py:81-138   the kernel, sigma_f not squared                      admpc_gp_fit: K
 *   src/model_fitting/gp.py:325-345  fit: y_mean, K^-1 y                                   admpc_gp_fit: alpha, ymean
 *   src/model_fitting/gp.py:489-516  GPRegressor.save -> pickle -> gp_loader -> create    admpc_gp_install (no host in between)
 *   (the simulator behind ROS)       drive, record, fit offline, restart the node         admpc_rollout_observe_lane_batch
 *
 * A handle that is to learn is created with placeholder GPs (n_points = 0, which admpc.h admits): which kernels a handle runs is decided
 * at admpc_create from n_gp, so such a handle is on the GP paths from the start.  At N = 20 that is the same fused kernel F with the GP
 * loop in its shooting phase; at N = 40, 60 and 80 it is kernel R, the stage-wise Riccati kernel, in place of the segmented kernel S a
 * nominal handle gets (admpc_kernels.hip: use_seg; DESIGN section 7 has the step times of both).
 *
 * The host copy of a handle's configuration is NOT changed by an install.  Nothing on the host reads a GP's payload (Z, alpha, ymean,
 * sigma_f, inv_l2) after admpc_create: the host reads n_gp, N and the bounds, the kernels read the device copy.
 */
#ifndef ADMPC_LEARN_H
#define ADMPC_LEARN_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_fleet.h"
#include "admpc_lane.h"
#include "admpc_plant.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AdmpcGpBins {          /* 128 bytes: one regressor to learn */
    int32_t n_feat, feat[3], out;     /* as AdmpcGp: 1 .. 3 features, each in 3 .. 8; out in 3 .. 5                             */
    int32_t nb[3];                    /* bins per feature, >= 1; 1 for an unused feature; product <= ADMPC_GP_MAX_POINTS        */
    double  lo[3], hi[3];             /* the box of the grid, finite, hi > lo (used features)                                   */
    double  sigma_f, length[3];       /* > 0, finite (length: used features)                                                    */
    double  noise, count_noise;       /* diagonal of K: noise + count_noise / count_i; noise > 0, count_noise >= 0, finite      */
} AdmpcGpBins;

typedef struct AdmpcObserveParams {   /* 544 bytes */
    double  dt;                       /* > 0, finite: the period between two poses                                              */
    double  blend_min, blend_max;     /* the MODEL's speed band (what the solver is given as p); blend_max > blend_min          */
    int32_t substeps, n_gp;           /* RK4 steps per period in [1, 64]; regressors in [1, ADMPC_GP_MAX]                       */
    AdmpcGpBins gp[ADMPC_GP_MAX];
} AdmpcObserveParams;

/* The refusals of an AdmpcObserveParams, wherever one is taken, in this order: null; dt; the band; substeps; n_gp; then per regressor
 * n_feat, feat, out, nb (each >= 1, 1 where unused, product <= 32), lo / hi, sigma_f, length, noise, count_noise. */

/* prev [7][B] <- the seven pose arrays.  ADMPC_EINVAL: B < 0, a null array.  B == 0 is a no-op. */
int admpc_observe_latch_batch(int device, int B,
                              const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                              const double* yaw_rate, const double* steer, double* prev, void* stream);

/* What the model did not predict of the period that led from `prev` to the seven pose arrays (read-only here), and its statistics.
 * Two launches.
 *   1. admpc_observe_kernel, three lanes per vehicle as the plant kernel.  Per vehicle: u from (ack, mode) by rule 2 of admpc_plant.h
 *      with plant->brake_acc and the bounds of `model`; p = clip((prev v_x - blend_min) / (blend_max - blend_min), 0, 1) on the band of
 *      `obs`; x^ = `substeps` RK4 steps of h = obs->dt / substeps (one division) of model's configuration from prev, its GP included
 *      if it has one -- no clip, no v_min, no yaw wrap; y_j = (now_j - x^_j) / obs->dt for j = 3, 4, 5, every operation rounded on its
 *      own.  samples [B][10] <- prev v_x, v_y, yaw rate, steer, u0, u1 (feature index f reads entry f - 3), y_3, y_4, y_5, and 1.0 if
 *      these nine are all finite, else 0.0.  Then prev <- now, all seven rows, always.
 *   2. admpc_bin_kernel, one wave per (regressor g, bin).  A record is valid when its last entry is 1.0.  For a valid record and every
 *      used feature d: t_d = (z_d - lo_d) * s_d with s_d = nb_d / (hi_d - lo_d) formed once on the host, k_d = floor(t_d); accepted
 *      iff t_d >= 0 and k_d < nb_d for every d (z == lo is in, z == hi is out, NaN is out); bin = (k_0 * nb_1 + k_1) * nb_2 + k_2.
 *      bins [n_gp][32][5], in/out: count (a double), sum z_0, sum z_1, sum z_2 (0 for an unused feature), sum y_out.  The order of the
 *      sums is part of the contract: lane l of the wave adds records b = l, l + 64, ... in ascending order into its own partial sum
 *      from 0; then the 64 partial sums are added onto the stored value one after the other, lane 0 first; every operation rounded on
 *      its own.  dropped [ADMPC_GP_MAX + 1] int32, in/out: entry g grows by the valid records outside regressor g's box, the last
 *      entry by the records that are not valid.
 * ADMPC_EINVAL, in this order: obs as above; the plant parameters as admpc_plant_step_batch refuses them; a null model, B < 0; then
 * (B > 0) a null array.  B == 0 is a no-op. */
int admpc_observe_batch(const AdmpcSolver* model, const AdmpcPlantParams* plant, const AdmpcObserveParams* obs, int B,
                        const float* ack, const int32_t* mode,
                        const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                        const double* yaw_rate, const double* steer,
                        double* prev, double* samples, double* bins, int32_t* dropped, void* stream);

/* One wave per regressor: bins [n_gp][32][5] -> gp_out [n_gp], complete AdmpcGp records in device memory (unused entries zero,
 * inv_l2 = 1 / (length * length) formed on the host), and info [n_gp] int32.
 *   points  the bins with count >= min_count, in ascending bin order: Z_i = sum z / count, t_i = sum y / count.  Only the rows below the
 *           product of nb are read: what a larger grid left in the rows behind them is no point
 *   ymean   the serial sum of the t_i, divided by n
 *   K_ij    sigma_f * exp(-0.5 * sum_d (Z_i,d - Z_j,d)^2 * inv_l2_d) + delta_ij * (noise + count_noise / count_i), exp as the
 *           kernels evaluate it (model_dev.h: exp_nonpos); sigma_f is not squared
 *   alpha   K alpha = t - ymean by a Cholesky factorisation of the n x n matrix, one row per lane, the matrix in LDS
 *   failure pivot k (from 0) is not > 0 and finite, or point k's t is not finite (NaN statistics end here): the empty GP -- n_points 0,
 *           ymean 0, Z and alpha zero -- and info[g] = -(k + 1)
 *   success info[g] = n; n == 0 is a success with the empty GP
 * ADMPC_EINVAL, in this order: obs as above; min_count < 1; a null array. */
int admpc_gp_fit(int device, const AdmpcObserveParams* obs, int min_count, const double* bins, AdmpcGp* gp_out, int32_t* info,
                 void* stream);

/* Overwrites gp[0 .. n_gp) of the handle's DEVICE configuration with gp_dev [n_gp] (device memory, as admpc_gp_fit writes it), on
 * `stream`, by a one-wave kernel that checks each record: n_feat in 1 .. 3, the used feat in 3 .. 8, out in 3 .. 5, n_points in
 * 0 .. 32, and sigma_f, ymean and the used inv_l2, Z and alpha finite.  A record that fails is installed as the empty GP (n_feat 1,
 * feat 3, out 3, everything else zero: mean 0).  installed [n_gp] int32: 1 where the record was taken, 0 where it was replaced.
 * The caller orders the install against the solves of the handle (the same stream does).  A captured graph that solves on the handle
 * reads the new GP at its next replay: the kernels take the configuration by pointer.
 * ADMPC_EINVAL, in this order: a null handle; n_gp not the n_gp the handle was created with, or that is 0; a null array. */
int admpc_gp_install(AdmpcSolver* s, int n_gp, const AdmpcGp* gp_dev, int32_t* installed, void* stream);

/* admpc_rollout_lane_batch (admpc_plant.h) with every step observed: one latch of the poses, then T times a CALL of
 * admpc_rollout_lane_batch with T = 1 (traj advanced by one slot per step) and the two launches of admpc_observe_batch behind it.
 * `model` predicts (on the device of s); plant_model and plant move the vehicles as in the rollout.
 * ADMPC_EINVAL, in this order: obs as above; a null model; then the rollout's own refusals, reached by a call of it with an empty
 * batch; then a model on another device than s; then (B > 0 and T > 0) a null array, those of the rollout included. */
int admpc_rollout_observe_lane_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcLaneParams* lane, const AdmpcStepParams* prm,
                                     const AdmpcSolver* plant_model, const AdmpcPlantParams* plant, int B, int T,
                                     const int32_t* path_of, int32_t* lane_idx,
                                     double* px, double* py, double* yaw, double* vx, double* vy, double* yaw_rate, double* steer,
                                     double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid, void* work,
                                     float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost,
                                     double* tally, int32_t* counts, double* traj,
                                     const AdmpcSolver* model, const AdmpcObserveParams* obs,
                                     double* prev, double* samples, double* bins, int32_t* dropped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_LEARN_H */
