/*
 * admpc_quad_noise.h -- the simulator's random disturbances on the device (libadmpc.so; csrc/admpc_quad_noise.hip, the plant step csrc/admpc_quad_plant.hip): the plant step and
 * the closed-loop rollout of admpc_quad_fleet.h / admpc_quad_learn.h under `noisy` (a normal force and torque per sub-step) and
 * `motor_noise` (a normal error per rotor and sub-step), the reference's default data-collection set-up
 * (utils/configuration_parameters.py:47-50).  An addition to admpc_quad_fleet.h, whose conventions hold here: device pointers owned by
 * the caller, fp64; `stream` a hipStream_t passed as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for
 * the message; the caller's HIP device restored; no host synchronisation and no allocation in the batch entries, which can be captured
 * into a graph.  Every refusal listed below comes in front of the first device call, in the order it is listed.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                             replaced by
 *   -----------------------------------------------------------------------------------  ------------------------------------
 *   quad_mpc/quad_3d.py:187-202    the draws of an update: four rotors, f_d, t_d           AdmpcQuadNoiseParams, the draws below
 *   quad_mpc/quad_3d.py:207-215    the RK4 stages under one f_d, t_d                       } admpc_quad_plant_step_noise_batch
 *   quad_mpc/quad_3d.py:271        f_vel: R(q) (a_thrust + f_d / mass)                     }
 *   quad_mpc/quad_3d.py:284-286    f_rate: thrust . y_f + t_d[0] + ..., and the two others }
 *   experiments/comparative_experiment.py:265-273  every model flown against these         admpc_quad_rollout_noise_batch
 *
 * NOT offered: np.random's own stream.  The DISTRIBUTIONS are the reference's, at the same places of Quadrotor3D.update; the numbers
 * come from a counter-based generator, so that this contract says which number every vehicle, period and sub-step gets.
 *
 * THE DRAWS.  Vehicle b of the batch in period p = noise_step[b] gets ten standard normals z[0 .. 9] at sub-step m (0 <= m < substeps
 * <= 1024), from five calls j = 0 .. 4 of Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53 and 0xCD9E8D57, Weyl constants
 * 0x9E3779B9 and 0xBB67AE85) with
 *     counter (b, p & 0xffffffff, p >> 32, 8 * m + j)       key (seed & 0xffffffff, seed >> 32).
 * The output words o0 .. o3 give w0 = o0 | o1 << 32 and w1 = o2 | o3 << 32, and
 *     u_k = ((double)(w_k >> 11) + 0.5) * 0x1p-53,   r = sqrt(-2.0 * log(u_0)),   a = 6.283185307179586 * u_1,
 *     z[2j] = r * cos(a),   z[2j + 1] = r * sin(a),
 * every operation rounded on its own (no contraction).  u_0 > 0 always, so r is finite and at most 8.66.  The integer part is exact;
 * log, cos and sin are the device library's (2 ulp each), so z agrees with another IEEE implementation to about 6 ulp of r (measured
 * against numpy on 67 x 40 x 10 draws: 1.0 ulp of max(1, r)).
 * z[0 .. 3] go to rotors 0 .. 3, z[4 .. 6] to f_d, z[7 .. 9] to t_d.  A switch that is off leaves its draws unused; the other switch's
 * numbers do not change.
 *
 * THE SUB-STEP.  With a_i the clipped commanded activation (rule 1 of admpc_quad_plant_step_batch; a non-finite one becomes u_min and
 * is counted):
 *   motor_noise  per sub-step  n_i = motor_bias * (a_i / motor_ref)^2 + motor_std * sqrt(a_i) * z[i]   and
 *                thrust_i = max(min(a_i - n_i, u_max), u_min) * max_thrust  (:189-192);   otherwise thrust_i = a_i * max_thrust
 *   noisy        f_d = force_std * z[4 .. 6], t_d = torque_std * z[7 .. 9], constant over the four RK4 stages of the sub-step (:198-199)
 *   f_vel   becomes  ... + R(q) ([0, 0, sum(thrust) / mass] + f_d / mass)
 *   f_rate  becomes  (thrust . y_f + t_d[0] + (J1 - J2) w1 w2) / J0, and the other two rows likewise
 * and everything else, unit_quat included, is the deterministic sub-step of admpc_quad_plant_step_batch.
 *
 * noise_step [B] uint64 in device memory, owned by the caller: vehicle b's period counter.  Vehicle b's own lane writes it back as
 * p + 1 behind the period, so a captured rollout draws fresh numbers at every replay.
 *
 * Measured on one MI355X at B = 4096, drag on, both switches on, noisy and deterministic alternating (profiles/HISTORY.md has every run):
 * a closed-loop step 532.5 against 451.0 us at N = 10 (40 sub-steps) and 1479.8 against 1436.3 us at N = 20 (20 sub-steps); the plant
 * kernel by trace 146.3 against 66.4 us and 79.7 against 36.7 us.
 */
#ifndef ADMPC_QUAD_NOISE_H
#define ADMPC_QUAD_NOISE_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_quad.h"
#include "admpc_quad_fleet.h"
#include "admpc_quad_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AdmpcQuadNoiseParams {      /* 56 bytes */
    uint64_t seed;                         /* the Philox key: (low 32 bits, high 32 bits) */
    int32_t  noisy, motor_noise;           /* 0 / 1 each; at least one of them 1 */
    double   force_std, torque_std;        /* >= 0, finite: std of every component of f_d [N] and t_d [N m] of ONE sub-step; the reference: 10 * dt (:198-199) */
    double   motor_bias, motor_ref, motor_std;   /* finite, motor_ref > 0, motor_std >= 0; the reference: 0.1, 1.3, 0.02 (:190-191) */
} AdmpcQuadNoiseParams;

/* The ten normals of every (vehicle, sub-step) of ONE period, for the host: z [B][substeps][10] doubles; raw NULL or
 * [B][substeps][10] uint64: the ten w words (w0, w1 of j = 0 .. 4).  noise_step is read, not advanced.  All ten are written whatever
 * the switches say.  One thread per (vehicle, sub-step), through the device function the plant uses.
 * ADMPC_EINVAL, in this order: a null noise; a switch that is not 0 or 1; both switches 0; force_std, torque_std or motor_std negative
 * or not finite; motor_ref not positive or not finite, or motor_bias not finite; B < 0; substeps outside [1, 1024]; then (B > 0) a
 * null noise_step or z.  B == 0 is a no-op.  ADMPC_ENODEV: no such device. */
int admpc_quad_noise_draw_batch(const AdmpcQuadNoiseParams* noise, int device, int B, int substeps, const uint64_t* noise_step,
                                double* z, uint64_t* raw, void* stream);

/* admpc_quad_plant_step_batch under the disturbances: plant->substeps noisy sub-steps under one input, for B vehicles in place, and
 * noise_step[b] <- noise_step[b] + 1.  Up to 8192 vehicles each gets four lanes, which share out the generator's calls and hand the
 * normals to the integrating lane through LDS; beyond, one lane per vehicle.  The mapping changes no result.
 * ADMPC_EINVAL, in this order: the plant parameters as in admpc_quad_plant_step_batch; a null noise; a switch that is not 0 or 1; both
 * switches 0 ("call admpc_quad_plant_step_batch"); force_std, torque_std or motor_std negative or not finite; motor_ref not positive or
 * not finite, or motor_bias not finite; motor_noise with plant->u_min < 0 (the reference takes sqrt(u_i)); then B < 0; then (B > 0) a
 * null u or x, u_stride < 4; a null noise_step.  B == 0 is a no-op.  ADMPC_ENODEV: no such device. */
int admpc_quad_plant_step_noise_batch(const AdmpcQuadPlantParams* plant, const AdmpcQuadNoiseParams* noise, int device, int B,
                                      const double* u, int64_t u_stride, double* x, uint64_t* noise_step, void* stream);

/* T closed-loop steps under the disturbances: step for step the chain of admpc_quad_rollout_batch -- or, with a model, of
 * admpc_quad_rollout_observe_batch -- with the plant launch replaced by the noisy one.  The arguments up to u_out are
 * admpc_quad_rollout_batch's; model, obs, prev, samples, bins, dropped are admpc_quad_rollout_observe_batch's (model == NULL: not
 * observed, and the five behind it are not read).  Tally, counts, traj_out, u_out and the idx advance are unchanged: u_out stays the raw
 * ubar[b][0], and the observation keeps recording the COMMANDED, clipped activations -- what the reference records -- so the motor bias
 * ends up in the residual the GP learns.  noise_step[b] advances by T.
 * ADMPC_EINVAL, in this order: the plant parameters; the disturbances and motor_noise with u_min < 0 as in
 * admpc_quad_plant_step_noise_batch; then every refusal of the entry it extends, in that entry's order and under that entry's name;
 * a null noise_step.  B == 0 and T == 0 are no-ops. */
int admpc_quad_rollout_noise_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B,
                                   int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                   double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                   double* tally, int32_t* counts, double* traj_out, double* u_out,
                                   const AdmpcQuadSolver* model, const AdmpcQuadObserveParams* obs,
                                   double* prev, double* samples, double* bins, int32_t* dropped,
                                   const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_NOISE_H */
