/*
 * admpc_quad_learn.h -- fitting the body-frame residual GPs of a quadrotor handle on the device from the steps a fleet has flown:
 * observe -> bin -> fit -> install (libadmpc.so; csrc/admpc_quad_learn.hip).  An addition to admpc_quad.h, admpc_quad_fleet.h and
 * admpc_learn.h, whose conventions hold here: device pointers owned by the caller, instance-major and dense, fp64; `stream` a hipStream_t
 * passed as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message; the caller's HIP device
 * restored; no host synchronisation and no allocation in the batch entries; every refusal in front of the first device call, in the
 * order it is listed; B == 0 and T == 0 are no-ops.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                 replaced by
 *   ---------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp_common.py:68-99   load_data: state_in, state_pred and state_out mapped    admpc_quad_observe_batch: samples
 *                                      to the body frame, y_err = (x_out - x_pred) / dt
 *   model_fitting/gp_common.py:101-112 prune_dataset: the data set cut into bins               admpc_quad_observe_batch: bins
 *   model_fitting/gp.py:81-138, 325-345  the kernel (sigma_f not squared); fit: y_mean, K^-1 y admpc_quad_gp_fit
 *   experiments/point_tracking_and_record.py:215-265  of the recording loop the RECORD of a    admpc_quad_rollout_observe_batch (along the
 *                                      flown period (:215, :230-234, :261-265): predict with    trajectories of a bank); the FLIGHT of that loop
 *                                      the nominal model, store state_in, input_in, state_out   -- random targets, the reach test per sub-step,
 *                                      and state_pred                                           the recovery, the period a vehicle really flew
 *                                                                                               -- is admpc_quad_targets.h's
 *   quad_mpc/quad_3d_optimizer.py:289-327  where the GP enters the model of the MPC            admpc_quad_gp_install (no host in between)
 *
 * NOT offered:
 *   - the evaluation of the learned GPs on a data set (gp_fitting.py:304-348 gp_evaluate_test_set), the posterior standard deviation
 *     among it, by THESE entries: admpc_quad_eval.h has it over a log of these records, for a clustered ensemble;
 *   - the search of the hyperparameters by THESE entries: to admpc_quad_gp_fit the length scales, sigma_f and the noise are GIVEN, as in
 *     admpc_learn.h; admpc_quad_hyper.h has the search (admpc_quad_gp_search, admpc_quad_gp_refit), routed to the kernels of
 *     admpc_hyper.h through the AdmpcGpBins that AdmpcQuadObserveParams holds as AdmpcObserveParams does;
 *   - clustered GP ensembles by THESE entries (one handle and one block of regressors, as in admpc_quad_fleet.h): admpc_quad_ensemble.h
 *     has observe -> bin -> fit -> install per cluster, and the rollout that flies them;
 *   - np.random's own stream for the simulator's random disturbances: their distributions are flown by admpc_quad_rollout_noise_batch
 *     (admpc_quad_noise.h), observed or not, from a counter-based generator;
 *   - handles in SQP mode (the rollout is the RTI loop).  The SQP loop inside the solve kernel, set on an RTI handle by admpc_quad_set_sqp of
 *     admpc_quad_sqp.h, is served by the observed rollout as it stands;
 *   - pruning by a velocity cap and by the error histograms (gp_common.py:101-112) by THESE entries, beyond what the box of the bins does (a
 *     sample outside the box is dropped and counted): admpc_quad_prune.h has the reference's prune over a log of these records, which
 *     rewrites entry 13 -- a pruned record carries 2.0 there and is taken by no bin -- and the RDRv drag fit from what is left.
 *
 * A handle that is to learn is created with placeholder GPs (n_points = 0, which admpc_quad.h admits): the solve kernels take the GP path
 * from n_gp of the configuration, which an install does not change.  The host copy of a handle's configuration is NOT changed by an
 * install; nothing on the host reads a GP's payload after admpc_quad_create.
 *
 * Measured on one MI355X at B = 4096, drag on, three regressors of one feature on 32 bins (scripts/quad_learn_time.py):
 * a closed-loop step with observation takes 566.0 us against 518.5 us without at N = 10, 1617.8 against 1569.7 us at N = 20; the fit
 * with install 25 us; by kernel trace the observe kernel 5.8 us, the bin kernel 41.5 us, the fit kernel 13.7 us, the install kernel 5.9 us.
 */
#ifndef ADMPC_QUAD_LEARN_H
#define ADMPC_QUAD_LEARN_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_quad.h"
#include "admpc_quad_fleet.h"
#include "admpc_learn.h"      /* AdmpcGpBins */

#ifdef __cplusplus
extern "C" {
#endif

/* 400 bytes.  gp[g] is an AdmpcGpBins of admpc_learn.h as it stands, with the quadrotor's ranges: feat in 7 .. 16, indexing
 * z = [x with the velocity in the body frame; u] as AdmpcQuadConfig documents (7 .. 9 body-frame velocity, 10 .. 12 body rates, 13 .. 16
 * activations); out in 7 .. 9, the body-frame acceleration component. */
typedef struct AdmpcQuadObserveParams {
    double  dt;                       /* > 0, finite: the period between two states (the control period)                         */
    int32_t substeps, n_gp;           /* RK4 steps of the prediction per period in [1, 64]; regressors in [1, ADMPC_QUAD_GP_MAX]  */
    AdmpcGpBins gp[ADMPC_QUAD_GP_MAX];
} AdmpcQuadObserveParams;

/* The refusals of an AdmpcQuadObserveParams, wherever one is taken, in this order: null; dt; substeps; n_gp; then per regressor n_feat,
 * feat (7 .. 16), out (7 .. 9), nb (each >= 1, 1 where unused, product <= 32), lo / hi, sigma_f, length, noise, count_noise -- the
 * order and the conditions of admpc_learn.h. */

/* prev [B][13] <- x [B][13].  ADMPC_EINVAL: B < 0; then (B > 0) a null array.  B == 0 is a no-op. */
int admpc_quad_observe_latch_batch(int device, int B, const double* x, double* prev, void* stream);

/* What the model did not predict of the period that led from prev [B][13] to x [B][13] (read-only here) under the activations u, in
 * the body frame, and its statistics.  Two launches.
 *   1. admpc_quad_observe_kernel, one lane per vehicle, as the plant kernel maps it.  Per vehicle b:
 *      a_i = max(min(u_i, plant->u_max), plant->u_min), a non-finite u_i becomes plant->u_min: rule 1 of admpc_quad_plant_step_batch,
 *      u row b at u + b * u_stride.  Nothing else of `plant` is read.
 *      x^ = `substeps` classic RK4 steps of h = obs->dt / substeps (one division) from prev[b] under a, of the configuration of `model` as
 *      it stands in its DEVICE copy: rdrv and the GPs included, the GP features and the rotation of the means from the integrated state
 *      (as gp_state = NULL does away from node 0).  The model text is the solve's (csrc/quad_model_dev.h).  No quaternion projection.
 *      The body-frame map of a state s:  v_b,i(s) = (R[0][i] * v_0 + R[1][i] * v_1) + R[2][i] * v_2  with R the rotation matrix of s's
 *      OWN quaternion in the expressions of quad_rot (utils.py:323-338; world_to_body_velocity_mapping takes it so), every operation
 *      rounded on its own (no contraction).
 *      samples [B][14] <- v_b(prev) (3), the body rates of prev (3), a (4), y_j = (v_b,j(x[b]) - v_b,j(x^)) / obs->dt for j = 0, 1, 2,
 *      and 1.0 if these thirteen are all finite, else 0.0.  Feature index f reads entry f - 7, output `out` reads entry 10 + out - 7.
 *      Then prev[b] <- x[b], always.
 *   2. admpc_quad_bin_kernel, one wave per (regressor g, bin): the contract of admpc_bin_kernel in admpc_learn.h (acceptance, the bin
 *      index, the lane-ordered sums: lane l adds b = l, l + 64, ... into its own partial sum from 0, then the 64 partial sums go onto the
 *      stored value one after the other, lane 0 first) with this record layout; the two kernels share one body (csrc/gp_fit_dev.h).
 *      bins [n_gp][32][5], in/out: count, sum z_0, sum z_1, sum z_2, sum y_out.  dropped [ADMPC_QUAD_GP_MAX + 1] int32, in/out: entry g
 *      grows by the valid records outside regressor g's box, the last entry by the records that are not valid.
 * ADMPC_EINVAL, in this order: obs as above; the plant parameters as admpc_quad_plant_step_batch refuses them; a null model; B < 0; then
 * (B > 0) a null array; u_stride < 4. */
int admpc_quad_observe_batch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B,
                             const double* u, int64_t u_stride, const double* x, double* prev, double* samples, double* bins,
                             int32_t* dropped, void* stream);

/* One wave per regressor: bins [n_gp][32][5] -> gp_out [n_gp], complete AdmpcGp records in device memory, and info [n_gp] int32 --
 * admpc_gp_fit of admpc_learn.h in every respect (points, ymean, K, the Cholesky solve, failure and success): the kernel's body is the
 * same text (csrc/gp_fit_dev.h), feat and out are written as given.
 * ADMPC_EINVAL, in this order: obs as above; min_count < 1; a null array. */
int admpc_quad_gp_fit(int device, const AdmpcQuadObserveParams* obs, int min_count, const double* bins, AdmpcGp* gp_out, int32_t* info,
                      void* stream);

/* Overwrites gp[0 .. n_gp) of the handle's DEVICE configuration with gp_dev [n_gp] (device memory, as admpc_quad_gp_fit writes it), on
 * `stream`, by a one-wave kernel that checks each record: n_feat in 1 .. 3, the used feat in 7 .. 16, out in 7 .. 9, n_points in
 * 0 .. 32, and sigma_f, ymean and the used inv_l2, Z and alpha finite.  A record that fails is installed as the empty GP (n_feat 1,
 * feat 7, out 7, everything else zero: mean 0).  installed [n_gp] int32: 1 where the record was taken, 0 where it was replaced.  The
 * record is written in 8-byte words.  The caller orders the install against the solves of the handle (the same stream does).  A
 * captured graph that solves on the handle reads the new GP at its next replay: the kernels take the configuration by pointer.
 * ADMPC_EINVAL, in this order: a null handle; n_gp not the n_gp the handle was created with, or that is 0; a null array. */
int admpc_quad_gp_install(AdmpcQuadSolver* s, int n_gp, const AdmpcGp* gp_dev, int32_t* installed, void* stream);

/* admpc_quad_rollout_batch (admpc_quad_fleet.h) with every step observed: one latch of x, then T times a CALL of admpc_quad_rollout_batch
 * with T = 1 (traj_out and u_out advanced by one slot per step) and the two launches of admpc_quad_observe_batch behind it, under ubar
 * with stride N * 4: the activations the plant has just applied.  `model` predicts; it is the controller's own handle or another one
 * (a nominal one: then the samples are what the controller's GPs are to learn).
 * ADMPC_EINVAL, in this order: obs as above; a null model; then the rollout's own refusals, reached by a call of it with an empty batch;
 * then a model on another device than s; then (B > 0 and T > 0) a null array, those of the rollout included. */
int admpc_quad_rollout_observe_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B,
                                     int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                     double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                     double* tally, int32_t* counts, double* traj_out, double* u_out,
                                     const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs,
                                     double* prev, double* samples, double* bins, int32_t* dropped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_LEARN_H */
