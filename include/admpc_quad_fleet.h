/*
 * admpc_quad_fleet.h -- the quadrotor's closed loop on the device (libadmpc.so; csrc/admpc_quad_fleet.hip, the plant step csrc/admpc_quad_plant.hip): the simplified simulator as a
 * PLANT step, a bank of over-sampled reference trajectories, the reference window of every vehicle, and T closed-loop steps of
 * window -> RTI step -> plant per call, with a tally of the tracking error.  An addition to admpc_quad.h, whose conventions hold here:
 * device pointers owned by the caller, instance-major and dense, fp64; `stream` a hipStream_t passed as void*; 0 or a negative ADMPC_E*
 * code returned, admpc_last_error() of admpc.h for the message; the caller's HIP device restored; no host synchronisation and no
 * allocation in the batch entries.  Every refusal listed below comes in front of the first device call, in the order it is listed.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                             replaced by
 *   -----------------------------------------------------------------------------------  ------------------------------------
 *   quad_mpc/quad_3d.py:22-95      the simulator's vehicle: mass, J, arms, drag, payload   AdmpcQuadPlantParams
 *   quad_mpc/quad_3d.py:175-220    Quadrotor3D.update: clip, RK4 over f_pos / f_att /       } admpc_quad_plant_step_batch
 *   quad_mpc/quad_3d.py:222-287    f_vel / f_rate, unit_quat                                }
 *   experiments/trajectory_test.py:114-119  control_period / simulation_dt updates per step  plant.substeps
 *   utils/quad_3d_opt_utils.py:267-296      get_reference_chunk                             } admpc_quad_ref_chunk_batch
 *   quad_mpc/quad_3d_optimizer.py:465-503   set_reference_trajectory: last-row padding      }
 *   experiments/trajectory_test.py:94-127   the loop: window, optimize, simulate, next index admpc_quad_rollout_batch
 *   experiments/trajectory_test.py:137      mean of the position error norms (the "RMSE")   tally[b][0] / counts[b][0]
 *   quad_mpc/quad_3d_optimizer.py:29-207    (the horizon and device of a built solver)      admpc_quad_solver_info
 *
 * The plant here is the deterministic simulator.  The simulator's random disturbances (`noisy`: a normal force and torque per sub-step;
 * `motor_noise`: a normal error per rotor and sub-step, quad_3d.py:187-202) are flown by the entries of admpc_quad_noise.h, which has
 * their distributions at the same places of the update.  NOT offered: np.random's own stream; the numbers come from a counter-based
 * generator that the contract there spells out.
 */
#ifndef ADMPC_QUAD_FLEET_H
#define ADMPC_QUAD_FLEET_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_quad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The SIMULATOR's vehicle (Quadrotor3D), which is not the controller's (AdmpcQuadConfig): it has the drag and the payload the
 * controller's model does not know.  Passed by value into the kernel.  216 bytes. */
typedef struct AdmpcQuadPlantParams {
    double  dt;                 /* > 0, finite: simulation_dt, the length of one sub-step (trajectory_test.py: 5e-4)           */
    double  mass;               /* > 0   quad_3d.py:59                                                                         */
    double  J[3];               /* > 0   quad_3d.py:58                                                                         */
    double  max_thrust;         /*       quad_3d.py:39   N per rotor at activation 1                                           */
    double  x_f[4], y_f[4], z_l_tau[4];   /* quad_3d.py:64-75  rotor arms, yaw-torque coefficients                             */
    double  g;                  /*       quad_3d.py:78   9.81                                                                  */
    double  rotor_drag[3];      /*       quad_3d.py:85-87  (rotor_drag_xy, rotor_drag_xy, rotor_drag_z)                        */
    double  aero_drag;          /*       quad_3d.py:88                                                                         */
    double  payload_mass;       /*       quad_3d.py:94-95  0 without a payload                                                 */
    double  u_min, u_max;       /* u_min <= u_max, finite: min_input_value, max_input_value (quad_3d.py:54-55)                 */
    int32_t substeps;           /* in [1, 1024]: updates per call, all under one input (control_period / simulation_dt)        */
    int32_t drag;               /* 0 / 1: quad_3d.py:90; with 0, rotor_drag and aero_drag are not read                         */
} AdmpcQuadPlantParams;

/* Quadrotor3D.update(u, dt) `substeps` times under one input, for B vehicles in place.  Per vehicle:
 *   1. a_i = max(min(u_i, u_max), u_min), thrust_i = a_i * max_thrust  (:184-194).  DEVIATION: an activation that is not finite is
 *      replaced by u_min (Python's max(min(NaN, hi), lo) gives lo, but min(hi, NaN)-style orders give NaN: the reference's result depends
 *      on the argument order of a builtin; here it is u_min, and the rollout counts the step).
 *   2. `substeps` times: classic RK4 with step dt over
 *        p' = v                                                          f_pos  (:222-230)
 *        q' = 1/2 skew_symmetric(w) q, the 4 x 4 form of utils.py:392    f_att  (:232-242)
 *        v' = -g e_z - payload_mass * g / mass e_z + a_drag + R(q) [0, 0, sum(thrust) / mass]     f_vel  (:244-271)
 *             with drag: v_b = R(conj q) v;  a_b = -aero_drag * v_b^2 * sign(v_b) / mass - rotor_drag * v_b / mass (sign(0) = 0);
 *             a_drag = R(q) a_b;  without: 0
 *        w' = (thrust . y_f + (J1 - J2) w1 w2) / J0,  (-thrust . x_f + (J2 - J0) w2 w0) / J1,  (thrust . z_l_tau + (J0 - J1) w0 w1) / J2
 *                                                                         f_rate (:273-287)
 *      then q <- q / |q| (unit_quat, :218).
 * u [B] rows of 4 doubles, row b at u + b * u_stride (u_stride >= 4, in doubles: the rollout passes ubar itself with N * 4);
 * x [B][13] in/out.  One lane per vehicle.
 * ADMPC_EINVAL: a null plant; dt not positive or not finite; substeps outside [1, 1024]; mass or an entry of J not positive; u_min > u_max
 * or one of them not finite; drag neither 0 nor 1 (these before anything else is looked at); then B < 0; then (B > 0) a null array,
 * u_stride < 4.  B == 0 is a no-op.  ADMPC_ENODEV: no such device. */
int admpc_quad_plant_step_batch(const AdmpcQuadPlantParams* plant, int device, int B, const double* u, int64_t u_stride, double* x,
                                void* stream);

/* K reference trajectories in one device allocation: trajectory k has M[k] rows, traj[k] [M_k][13] states and u[k] [M_k][4] inputs
 * (HOST pointers; the over-sampled reference_traj / reference_u of trajectory_test.py:72-90).  Synchronous.
 * ADMPC_EINVAL: a null argument, K < 1, an M[k] < 1, a null traj[k] or u[k]. */
typedef struct AdmpcQuadTrajBank AdmpcQuadTrajBank;
int admpc_quad_traj_bank_create(int device, int K, const int32_t* M, const double* const* traj, const double* const* u,
                                AdmpcQuadTrajBank** bank);
void admpc_quad_traj_bank_destroy(AdmpcQuadTrajBank* bank);

/* get_reference_chunk(traj, u, idx, N, over) followed by set_reference_trajectory's padding with the last row, per vehicle.  With
 * M the length of trajectory traj_of[b], i = idx[b] and L = min(N + 1, ceil((M - i) / over)) the rows the window holds:
 *   yref[b][j]  = [ state row i + min(j, L - 1) * over ;  input row i + min(j, max(L - 2, 0)) * over ],   j = 0 .. N - 1
 *   yref_e[b]   =   state row i + min(N, L - 1) * over
 *   pos_ref[b]  =   entries 0 .. 2 of state row i                              (NULL: not written)
 * A vehicle with traj_of[b] outside [0, K) or idx[b] outside [0, M) gets NaN in all three: its solve reports status 4 and leaves its
 * iterate alone; its neighbours are not affected.  One thread per double written, so a node's 17 doubles leave contiguous lanes.
 * ADMPC_EINVAL: a null bank; B < 0; N outside [2, ADMPC_QUAD_MAX_N]; over < 1; then (B > 0) a null array. */
int admpc_quad_ref_chunk_batch(const AdmpcQuadTrajBank* bank, int B, int N, int over, const int32_t* traj_of, const int32_t* idx,
                               double* yref, double* yref_e, double* pos_ref, void* stream);

/* T closed-loop steps on `stream`, the loop of trajectory_test.py:94-127 for B vehicles.  Each step is one chain of three launches:
 *   1. admpc_quad_ref_chunk_batch into yref / yref_e (the position reference of the tally is yref[b][0][0:3], the position of row idx);
 *   2. admpc_quad_solve_batch_ex(s, B, x, yref, yref_e, NULL, xbar, ubar, cost, status, iters): x is x0, the GP state defaults to it; the
 *      iterate xbar / ubar is persistent and never shifted, as in the reference;
 *   3. the plant step under ubar[b][0] as it stands after the solve -- whatever the status: trajectory_test.py does not look at it
 *      either -- with the tally, the counts, the records and idx[b] <- min(idx[b] + 1, M - 1) in the same launch.
 *   idx       [B] int32 in/out.  A vehicle whose traj_of or idx is out of range keeps its idx.
 *   yref [B][N][17], yref_e [B][13]                  work arrays: the window of the last step on return
 *   cost [B], status [B] int32, iters [B] int32      of the last step; status must be given, cost and iters may be NULL
 *   tally  [B][3] double, in/out, zeroed by the caller: sum of |e|, sum of |e|^2, max of |e| with e = pos_ref - x[0:3] at the START of
 *          the step, pos_ref the position of row idx (sum |e| / steps is the figure trajectory_test.py:137 prints).  |e|^2 = (ex * ex + ey * ey) + ez * ez, |e| its square
 *          root, every operation rounded on its own (no contraction), the sums serial over the steps; a step whose |e|^2 is not finite
 *          adds nothing.
 *   counts [B][3] int32, in/out: steps taken; steps with status != 0; steps in which an activation was replaced (not finite).
 *   traj_out  NULL or [T + 1][B][13]: slot t holds x at the start of step t, slot T the final state.
 *   u_out     NULL or [T][B][4]: ubar[b][0] of step t as the solve left it (before the plant's clip).
 * No host synchronisation and no allocation between the steps.  The N = 20 handle allocates its slot buffer at its FIRST solve, so the
 * chain can be captured into a graph once one solve has run on the handle.  If an enqueue fails in the middle the error is returned;
 * the steps already enqueued run.  T == 0 or B == 0 is a no-op.
 * NOT served: handles in SQP mode (the rollout is the RTI loop of trajectory_test.py).  The SQP loop inside the solve kernel, set on an RTI
 * handle by admpc_quad_set_sqp of admpc_quad_sqp.h, is served by this chain as it stands.  One handle drives the whole fleet here;
 * clustered GP ensembles are flown by admpc_quad_ensemble_rollout_batch of admpc_quad_ensemble.h, which is this chain with the routing
 * from the window and admpc_quad_solve_batch_routed in place of step 2.
 * ADMPC_EINVAL, in this order: a null solver; a solver with sqp_iters > 1; a null bank; a bank on another device than the solver; the
 * plant parameters as in admpc_quad_plant_step_batch; over < 1; B < 0; T outside [0, 4096]; then (B > 0 and T > 0) a null array among
 * traj_of .. status, tally or counts. */
int admpc_quad_rollout_batch(AdmpcQuadSolver* s, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over, int B, int T,
                             const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                             double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                             double* tally, int32_t* counts, double* traj_out, double* u_out, void* stream);

/* What the rollout needs of a built solver (defined in csrc/admpc_quad.hip): its device, horizon and sqp_iters; each pointer may be
 * NULL.  ADMPC_EINVAL: a null solver. */
int admpc_quad_solver_info(const AdmpcQuadSolver* s, int* device, int* N, int* sqp_iters);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_FLEET_H */
