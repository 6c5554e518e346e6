/*
 * admpc_plant.h -- a PLANT step on the device, and T closed-loop steps along a route per call (libadmpc.so; csrc/admpc_plant.hip,
 * csrc/admpc_step.hip).  An addition to admpc.h, admpc_fleet.h and admpc_lane.h, whose conventions hold here: device pointers owned by
 * the caller, `stream` a hipStream_t passed as void*, 0 or a negative ADMPC_E* code returned, admpc_last_error() for the message, the
 * caller's HIP device restored, no host synchronisation and no allocation.
 *
 * The reference has no car plant: AD3D.update is commented out (ad_3d.py:109) because its plant is a simulator behind ROS.  The entry
 * points below move the vehicles under the record the control step issued, with the model the controller itself integrates:
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/...)                                replaced by
 *   ----------------------------------------------------------------------------------  ------------------------------------
 *   src/ad_mpc/ad_3d_optimizer.py:280-310  the model f(x, u, p), GP residual included     } one classic RK4 step per sub-step,
 *   acados ERK4 (acados_solver_sim_car.c:655-665)                                         } admpc_plant_step_batch
 *   src/ad_mpc/create_ros_ad_mpc.py:96,98   acceleration and steering-angle velocity of   the inputs of an MPC record (mode == 1)
 *                                           the record are w_opt[0:2]
 *   nodes/gp_ad_mpc_node.py:455-476         the auxiliary controller's brake record        the inputs of every other record
 *   src/ad_mpc/ref_traj.py:28               bound_angle_within_pi                          the yaw at the end of the period
 *   (the simulator behind ROS)              pose message -> command -> next pose message   admpc_rollout_lane_batch
 */
#ifndef ADMPC_PLANT_H
#define ADMPC_PLANT_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_fleet.h"
#include "admpc_lane.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AdmpcPlantParams {      /* 48 bytes */
    double  dt;                    /* > 0: the period a command is held for (FleetController: opt_dt)                    */
    double  blend_min, blend_max;  /* the PLANT's speed band: p = clip((v_x - blend_min) / (blend_max - blend_min), 0, 1),
                                      taken once, at the start of the period (host.vel_switch); blend_max > blend_min  */
    double  brake_acc;             /* <= 0: acceleration under a brake record (mode != 1); raised to cfg lbu[0] if below  */
    double  v_min;                 /* >= 0: v_x is raised to v_min after every sub-step                                  */
    int32_t substeps;              /* M in [1, 64]: classic RK4 steps of h = dt / M (one division, in double)            */
    int32_t reserved;              /* 0                                                                                  */
} AdmpcPlantParams;

/* Advances the seven states of every vehicle in place by one control period, under the record the step issued: ack [B][4] float32 and
 * mode [B] as admpc_control_step_*_batch write them.  `model` supplies the vehicle constants, the input and steering bounds and the GP
 * residual, if its configuration carries one; its horizon and weights are not read.  Per vehicle, in this order:
 *   1. x = [px, py, yaw, vx, vy, yaw_rate, steer]; the plant's band gives p from x[3] (NaN kept).
 *   2. mode == 1 and ack[3], ack[1] both finite: u0 = clip((double)ack[3], lbu[0], ubu[0]), u1 = clip((double)ack[1], lbu[1], ubu[1]);
 *      otherwise the brake record: u0 = max(brake_acc, lbu[0]), u1 = 0 (the steering is held).
 *   3. M times: x <- RK4(f(., u, p), h), the step of the model the solver shoots with; then x[6] is clipped to [lbx_delta, ubx_delta];
 *      then x[3] is raised to v_min.
 *   4. once: yaw = (yaw + pi) % (2 pi) - pi with the floor modulo (fmod, plus 2 pi when the result is negative), the constants M_PI
 *      and 2.0 * M_PI, every operation rounded on its own.
 * Three lanes per vehicle, as in the shooting kernels (they share the sums of the GP residual).
 * ADMPC_EINVAL, all in front of the first device call: a null plant, dt not positive or not finite, blend_max <= blend_min,
 * brake_acc > 0, v_min < 0, substeps outside [1, 64] (these before anything else is looked at); then a null model, B < 0, a null
 * array.  B == 0 is a no-op. */
int admpc_plant_step_batch(const AdmpcSolver* model, const AdmpcPlantParams* plant, int B,
                           const float* ack, const int32_t* mode,
                           double* px, double* py, double* yaw, double* vx, double* vy, double* yaw_rate, double* steer,
                           void* stream);

/* T closed-loop steps on `stream`: each is the chain of admpc_control_step_lane_batch (admpc_lane.h), launch for launch, and one launch
 * behind it that does the plant step above and the tally.  No host synchronisation between the steps: the whole rollout can be captured
 * into a graph once admpc_reserve(s, B) has run.  The arrays of the lane step keep their meaning, except that the pose arrays are
 * in/out; ack ... cost hold the values of the last step.
 *   plant_model  NULL: s.  A plant model on another device than s is refused.
 *   tally  [B][3] double, in/out, zeroed by the caller: sum of e_y^2, sum of e_psi^2, max of |e_y|, where e_y and e_psi are entries 1
 *          and 2 of the step's out_err (the generator's own tracking errors at the pose the step saw).  The sums run serially over the
 *          steps, every operation rounded on its own; a step whose e_y or e_psi is not finite adds nothing.
 *   counts [B][3] int32, in/out: the steps taken, the steps with mode == 1, the unusable steps (status != 0 || valid == 0).
 *   traj   NULL or [T + 1][7][B]: slot t holds the seven pose arrays at the start of step t, slot T the final state.
 * A vehicle with path_of[b] outside the bank behaves as the lane step defines (status 4, brake record, lane_idx untouched): the plant
 * brakes it, its tally stays untouched (its errors are NaN) and its counts[2] grows by one per step.
 * T == 0 or B == 0 is a no-op.  If an enqueue fails in the middle the error is returned; the steps already enqueued run.
 * ADMPC_EINVAL, in this order: the lane parameters as in the lane step; the plant parameters as above; the lane step's own refusals;
 * then T outside [0, 4096], a plant model on another device, a null tally or counts. */
int admpc_rollout_lane_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcLaneParams* lane, const AdmpcStepParams* prm,
                             const AdmpcSolver* plant_model, const AdmpcPlantParams* plant, int B, int T,
                             const int32_t* path_of, int32_t* lane_idx,
                             double* px, double* py, double* yaw, double* vx, double* vy, double* yaw_rate, double* steer,
                             double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid, void* work,
                             float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost,
                             double* tally, int32_t* counts, double* traj, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_PLANT_H */
