/*
 * admpc_quad_targets.h -- flying to random target points and recording, on the device (libadmpc.so; csrc/admpc_quad_targets.hip, the plant step csrc/admpc_quad_plant.hip, the observation csrc/admpc_quad_learn.hip): a
 * point reference for every vehicle, the reach test after every simulator sub-step, the sampling of the next target, the recovery of a
 * vehicle that has run away, and an observation whose period is the time a vehicle really flew.  An addition to admpc_quad_fleet.h,
 * admpc_quad_learn.h and admpc_quad_noise.h, whose conventions hold here: device pointers owned by the caller, fp64; `stream` a
 * hipStream_t passed as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message; the caller's HIP
 * device restored; no host synchronisation and no allocation in the batch entries, which can be captured into a graph.  Every refusal
 * listed below comes in front of the first device call, in the order it is listed.  B == 0 (and T == 0) is a no-op.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                              replaced by
 *   ------------------------------------------------------------------------------------  ------------------------------------
 *   experiments/point_tracking_and_record.py:82-107   sample_random_target                  } AdmpcQuadTargetParams, the rules below;
 *   experiments/point_tracking_and_record.py:112-125  world_radius, the first target        } admpc_quad_targets_reset_batch
 *   experiments/point_tracking_and_record.py:192-193  the point reference of the target     } admpc_quad_target_window_batch
 *   quad_mpc/quad_3d_optimizer.py:429-462             set_reference_state: one row, N times } (create_ros_gp_mpc.py hovers with it)
 *   experiments/point_tracking_and_record.py:204-206  the emergency recovery                admpc_quad_target_window_batch
 *   experiments/point_tracking_and_record.py:246-287  simulate until the period is over or  admpc_quad_plant_target_step_batch
 *                                                     the target is reached; the next target
 *   utils/utils.py:262-281                            euclidean_dist(target, p, thresh)     the reach test below
 *   experiments/point_tracking_and_record.py:215, 261-265  check_out_data with the flown    admpc_quad_observe_var_batch
 *                                                     simulation_time as dt
 *   experiments/point_tracking_and_record.py:187-294  the experiment's loop                 admpc_quad_rollout_targets_batch
 *
 * What each header replaces of that script: THIS one the flight (targets, reach, recovery, the variable period); admpc_quad_learn.h the
 * recording of a flown period (state_in, input_in, state_out, state_pred -> the sample) and everything behind it.
 *
 * NOT offered:
 *   - np.random's own stream: the DISTRIBUTIONS of sample_random_target are the reference's, the numbers come from the counter-based
 *     generator of admpc_quad_noise.h, so that this contract says which numbers every vehicle's every target takes;
 *   - SQP mode, although the reference's script asks for it: the RTI loop is what every rollout here flies.  That is a handle BUILT with
 *     sqp_iters > 1; the SQP loop inside the solve kernel, set on an RTI handle by admpc_quad_set_sqp of admpc_quad_sqp.h, is flown by
 *     admpc_quad_rollout_targets_batch as it stands, and tcounts[b][3] then counts status 2 as well;
 *   - clustered ensembles (admpc_quad_ensemble.h) and the logged rollout of admpc_quad_clusters.h;
 *   - the CSV data set and the real-time plot;
 *   - the reference's record of a period that ended in a recovery, which pairs the state before the recovery with the one after it: here
 *     the observation runs behind the plant, BEFORE the next period's recovery, records the flown period, and the recovery latches the
 *     state it sets.
 *
 * PER-VEHICLE STATE, device memory owned by the caller:
 *   target    [B][3] double   the target in force
 *   target_no [B] uint64      targets reached so far; it is the generator's counter: target number t is drawn with t
 *   n_iter    [B] int32       periods flown towards the target in force (:183, :258, :287)
 *   fast      [B] int32       1 iff the state at the start of the last flown period had a velocity component above v_max
 *   tcounts   [B][5] int32    targets reached; recoveries; periods flown; periods with status != 0; periods with a replaced activation
 *   presets   [B][n_preset][3] double, mode 0 only (read-only)
 * Every update of these is a plain store of the vehicle's own lane.
 *
 * THE RULES.  Every floating-point operation below is rounded on its own (no contraction).
 *
 * Reach (utils.py:276, point_tracking_and_record.py:255).  After each sub-step, with t the target and p = x[0 .. 2]:
 *     d = sqrt(((t0 - p0)^2 + (t1 - p1)^2) + (t2 - p2)^2),   reached iff d < thresh   (a NaN compares false).
 * The vehicle stops integrating at that sub-step: nsub[b] in 1 .. substeps is the number of sub-steps flown; a vehicle that has not
 * reached flies all plant->substeps.  At a reach target_no[b] += 1, tcounts[b][0] += 1, and the next target is installed in the same
 * launch, sampled from the position at the reach (:278).
 *
 * Iteration count (:258, :287).  Behind the period n_iter <- (reached ? 0 : n_iter) + 1.
 *
 * Recovery (:204-206).  At the start of a period, before the window: if fast[b] != 0 || n_iter[b] > max_iters then
 *     x[b] <- (target, 1, 0, 0, 0,  0, 0, 0,  0, 0, 0),  n_iter[b] <- 0,  tcounts[b][1] += 1,  prev[b] <- x[b] where prev is given.
 * fast[b] is written by the PLANT launch from the state at the START of its period: 1 iff x[7] > v_max || x[8] > v_max || x[9] > v_max
 * -- signed, as in the reference, and a NaN compares false.  So, as in the reference (whose `state` is of :208 one pass earlier), the
 * test sees the state of one period earlier.  admpc_quad_targets_reset_batch computes fast from the state it is given.
 *
 * Window (quad_3d_optimizer.py:429-462).  yref[b][j] = (target, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0) for j < N; yref_e[b] its first 13.
 *
 * Next target, modes 1 and 2 (:82-107).  Target number t = target_no[b] of vehicle b takes the calls j = 0, 1 of Philox4x32-10 with
 *     counter (b, t & 0xffffffff, t >> 32, 0xffffffff - j)       key (seed & 0xffffffff, seed >> 32),
 * the words w0, w1 of a call and u_k = ((double)(w_k >> 11) + 0.5) * 0x1p-53 as admpc_quad_noise.h forms them.  The disturbances' fourth
 * counter word is 8 * m + j <= 8188: the two streams cannot meet under one seed.  Three uniforms are used: u0 = u(w0 of call 0),
 * u1 = u(w1 of call 0), u2 = u(w0 of call 1).
 *     mode 1 ("aggressive", away from the position p):  theta = 6.283185307179586 * u0,  psi = 6.283185307179586 * u1,
 *             r = R + (u2 - 0.5) * R,   target = p + ((r * sin theta) * cos psi, (r * sin theta) * sin psi, r * cos theta)
 *     mode 2 (uniform in the world box):  target_k = -R + (2 * R) * u_k,  k = 0, 1, 2
 * with R = world_radius.  sin and cos are the device library's (2 ulp each): a target agrees with another IEEE implementation to a few
 * ulp of max(|p|, 1.5 R).
 *
 * Next target, mode 0.  Row target_no[b] of presets[b], while target_no[b] < n_preset.  A vehicle that has reached its last preset
 * (target_no[b] == n_preset) is DONE: it keeps that target, flies full periods without a reach test, is not recovered, and nothing of
 * n_iter and tcounts changes any more; fast and noise_step are still written.  The reference's loop ends there.
 *
 * Measured on one MI355X at B = 4096, drag on, the target flight and the flight along a circle alternating (scripts/quad_targets_time.py;
 * DESIGN section 7, profiles/HISTORY.md): by kernel trace over the periods of N = 10 and N = 20 the plant kernel towards targets takes 57.0 us
 * against 52.0 us of admpc_quad_plant_kernel, under the disturbances 120.3 against 113.4 us of the noisy plant kernel, the window
 * kernel 11.1 us against 8.3 us of the chunk kernel.  A closed-loop period of the target flight takes 1217 against 453 us at N = 10 and
 * 2903 against 1442 us at N = 20 (under the disturbances 844 against 533 and 2947 against 1487): the difference is the RTI step's, whose
 * interior point takes 8.9 to 9.3 iterations on average towards a point 1.5 to 4.5 m away, with the inputs at their bounds, and 3.0 along
 * a smooth circle.
 */
#ifndef ADMPC_QUAD_TARGETS_H
#define ADMPC_QUAD_TARGETS_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_quad.h"
#include "admpc_quad_fleet.h"
#include "admpc_quad_learn.h"
#include "admpc_quad_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AdmpcQuadTargetParams {     /* 48 bytes; passed by value into the kernels */
    uint64_t seed;                         /* the Philox key: (low 32 bits, high 32 bits); not read in mode 0 */
    int32_t  mode;                         /* 0 presets, 1 random "aggressive" (away from the current position), 2 random uniform in the world box */
    int32_t  n_preset;                     /* mode 0: >= 1, the rows of presets[b]; otherwise not read */
    double   world_radius;                 /* > 0, finite; the reference: 3 (:112) */
    double   thresh;                       /* > 0, finite; the reference: 0.05 (:255) */
    double   v_max;                        /* not NaN; the reference: 14 (:204) */
    int32_t  max_iters;                    /* >= 0; the reference: 100 (:204) */
    int32_t  pad;
} AdmpcQuadTargetParams;

/* The refusals of an AdmpcQuadTargetParams, wherever one is taken, in this order: null; mode outside 0 .. 2; world_radius not positive or
 * not finite; thresh not positive or not finite; v_max NaN; max_iters < 0; mode 0 with n_preset < 1. */

/* The target that number target_no[b] gives vehicle b at position x[b][0 .. 2], for the host: target_out [B][3]; raw NULL or [B][4]
 * uint64, the words w0, w1 of calls 0 and 1.  x [B] rows of x_stride doubles (>= 3).  Nothing of the fleet's state is changed.
 * ADMPC_EINVAL, in this order: the target parameters; mode 0 ("the presets are not drawn"); B < 0; then (B > 0) a null x, target_no or
 * target_out; x_stride < 3.  ADMPC_ENODEV: no such device. */
int admpc_quad_target_draw_batch(const AdmpcQuadTargetParams* tp, int device, int B, const double* x, int64_t x_stride,
                                 const uint64_t* target_no, double* target_out, uint64_t* raw, void* stream);

/* target_no, n_iter and tcounts zeroed; fast from x [B][13] by the rule above; target number 0 sampled from x[b][0 .. 2] (modes 1, 2)
 * or row 0 of presets[b] (mode 0).
 * ADMPC_EINVAL, in this order: the target parameters; B < 0; then (B > 0) a null array among x, target, target_no, n_iter, fast and
 * tcounts; mode 0 with null presets.  ADMPC_ENODEV: no such device. */
int admpc_quad_targets_reset_batch(const AdmpcQuadTargetParams* tp, int device, int B, const double* x, const double* presets,
                                   double* target, uint64_t* target_no, int32_t* n_iter, int32_t* fast, int32_t* tcounts, void* stream);

/* The recovery and the window of a period, one launch (admpc_quad_target_window_kernel, one lane per vehicle): x [B][13] in/out,
 * n_iter and tcounts in/out, prev NULL or [B][13] (the latch of admpc_quad_learn.h, re-latched at a recovery), yref [B][N][17] and
 * yref_e [B][13] out.  target_no is read in mode 0 only (may be NULL otherwise).
 * ADMPC_EINVAL, in this order: the target parameters; B < 0; N outside [2, ADMPC_QUAD_MAX_N]; then (B > 0) a null array among x, target,
 * n_iter, fast, tcounts, yref and yref_e; mode 0 with a null target_no.  ADMPC_ENODEV: no such device. */
int admpc_quad_target_window_batch(const AdmpcQuadTargetParams* tp, int device, int B, int N, double* x, const double* target,
                                   const uint64_t* target_no, int32_t* n_iter, const int32_t* fast, int32_t* tcounts, double* prev,
                                   double* yref, double* yref_e, void* stream);

/* One period of the simulator towards the targets, one launch (admpc_quad_plant_period_kernel<NOISY, L, true>): per vehicle, in this order
 *   fast[b] from x[b]; the clip of the activations and `replaced` (rule 1 of admpc_quad_plant_step_batch); up to plant->substeps sub-steps
 *   of admpc_quad_plant_step_batch -- with `noise`, of admpc_quad_plant_step_noise_batch under the numbers that header gives (b,
 *   noise_step[b], sub-step m) -- with the reach test behind each; x[b] and nsub[b] written; then, unless the vehicle is DONE,
 *   tcounts[b][2] += 1, tcounts[b][3] += 1 where status is given and status[b] != 0, tcounts[b][4] += 1 where an activation was replaced,
 *   and at a reach target_no, tcounts[b][0] and the next target; n_iter by its rule; noise_step[b] += 1 whatever nsub[b] is.
 * noise and noise_step may be NULL: the deterministic simulator.  The noisy form gives a vehicle four lanes up to 8192 vehicles, which
 * share out the generator's calls through LDS as the noisy plant step does (the same kernel text without the targets); a vehicle that has reached keeps meeting the
 * barriers and only skips the integration.  The mapping changes no result.
 * u [B] rows of 4, row b at u + b * u_stride; x [B][13] in/out; status NULL or [B]; presets as above; nsub [B] int32 out.
 * ADMPC_EINVAL, in this order: the plant parameters as in admpc_quad_plant_step_batch; the target parameters; with a noise, its refusals
 * as in admpc_quad_plant_step_noise_batch; B < 0; then (B > 0) a null array among u, x, target, target_no, n_iter, fast, tcounts and nsub;
 * u_stride < 4; mode 0 with null presets; a noise with a null noise_step.  ADMPC_ENODEV: no such device. */
int admpc_quad_plant_target_step_batch(const AdmpcQuadPlantParams* plant, const AdmpcQuadTargetParams* tp, const AdmpcQuadNoiseParams* noise,
                                       int device, int B, const double* u, int64_t u_stride, double* x, const int32_t* status,
                                       const double* presets, double* target, uint64_t* target_no, int32_t* n_iter, int32_t* fast,
                                       int32_t* tcounts, int32_t* nsub, uint64_t* noise_step, void* stream);

/* admpc_quad_observe_batch with a period per vehicle: admpc_quad_observe_kernel<true> is admpc_quad_observe_kernel<false> with
 *     dt_b = obs->dt where nsub[b] == plant->substeps, else (double)nsub[b] * plant->dt;   h_b = dt_b / obs->substeps
 * in the places of obs->dt and h.  A record with nsub[b] < 1 is invalid (flag 0.0: counted in the last entry of dropped); prev is latched
 * all the same.  The bin launch behind it is admpc_quad_observe_batch's.  For a full period (nsub[b] == plant->substeps) this is the
 * existing record bit for bit.  The reference's dt is the accumulated `simulation_time` (:249): that differs from nsub * dt in the last
 * bits, and where control_period is no multiple of simulation_dt, by the overshoot of the last sub-step.
 * ADMPC_EINVAL, in this order: those of admpc_quad_observe_batch up to its arrays; then (B > 0) a null array, nsub included;
 * u_stride < 4. */
int admpc_quad_observe_var_batch(const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, const AdmpcQuadObserveParams* obs, int B,
                                 const double* u, int64_t u_stride, const double* x, double* prev, const int32_t* nsub, double* samples,
                                 double* bins, int32_t* dropped, void* stream);

/* T periods on `stream`, the loop of point_tracking_and_record.py:187-294 for B vehicles.  With a model, one latch of x first.  Each
 * period is a chain of
 *   1. admpc_quad_target_window_batch (prev: the model's latch, or NULL without a model);
 *   2. admpc_quad_solve_batch_ex(s, B, x, yref, yref_e, NULL, xbar, ubar, cost, status, iters): the iterate persistent, never shifted;
 *   3. admpc_quad_plant_target_step_batch under ubar[b][0] (stride N * 4), with status, and the records in the same launch;
 *   4. with a model: admpc_quad_observe_var_batch under the same activations and nsub.
 *   nsub       [B] int32 work array: of the last period on return
 *   traj_out   NULL or [T + 1][B][13]: slot 0 the state the first period starts from (behind its recovery), slot t + 1 the state period t
 *              leaves; a recovery at the start of period t + 1 is not in it (target_out[t + 1] is where the vehicle was put)
 *   u_out      NULL or [T][B][4]: ubar[b][0] as the solve left it
 *   nsub_out   NULL or [T][B] int32
 *   target_out NULL or [T][B][3]: the target in force during the period
 * model == NULL: not observed, obs .. dropped are not read.  noise == NULL: the deterministic simulator, noise_step is not read.
 * ADMPC_EINVAL, in this order: the plant parameters; the target parameters; with a noise, its refusals; with a model, obs as in
 * admpc_quad_learn.h; a null solver; a solver with sqp_iters > 1; B < 0; T outside [0, 4096]; a model on another device than s; then (B > 0
 * and T > 0) a null array among x, xbar, ubar, yref, yref_e, status, target, target_no, n_iter, fast, tcounts and nsub, and with a model
 * among prev, samples, bins and dropped; mode 0 with null presets; a noise with a null noise_step. */
int admpc_quad_rollout_targets_batch(AdmpcQuadSolver* s, const AdmpcQuadPlantParams* plant, const AdmpcQuadTargetParams* tp, int B, int T,
                                     double* x, double* xbar, double* ubar, double* yref, double* yref_e, double* cost, int32_t* status,
                                     int32_t* iters, const double* presets, double* target, uint64_t* target_no, int32_t* n_iter,
                                     int32_t* fast, int32_t* tcounts, int32_t* nsub, double* traj_out, double* u_out, int32_t* nsub_out,
                                     double* target_out, const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs, double* prev,
                                     double* samples, double* bins, int32_t* dropped, const AdmpcQuadNoiseParams* noise,
                                     uint64_t* noise_step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_TARGETS_H */
