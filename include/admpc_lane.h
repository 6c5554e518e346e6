/*
 * admpc_lane.h -- the fleet step along a ROUTE: a local lane per vehicle, cut on the device (libadmpc.so; csrc/admpc_lane.hip,
 * csrc/admpc_step.hip).  An addition to admpc.h and admpc_fleet.h, whose conventions hold here: device pointers owned by the caller,
 * `stream` a hipStream_t passed as void*, 0 or a negative ADMPC_E* code returned, admpc_last_error() for the message.
 *
 * RefTrajectory.get_waypoints lays its window from the path's FIRST waypoint on, whichever waypoint is closest (ref_traj.py:124-132:
 * start_dist is computed and never used).  The reference node gets away with that because its path is no route: it is the short local
 * lane of waypoint_callback, which begins at the vehicle, is clamped at the vehicle's speed, padded and handed to set_traj anew with
 * every message.  admpc_control_step_batch / _bank_batch inherit the generator and so serve vehicles near their path's start only.
 * The entry points below cut that local lane out of a route of the bank, per vehicle and per step:
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/...)                                replaced by
 *   ----------------------------------------------------------------------------------  ------------------------------------
 *   nodes/gp_ad_mpc_node.py:351-378   waypoint_callback: the lane that begins at the     the nearest-waypoint search and the cut of
 *                                     vehicle, padded with its last waypoint (:372-376)  L waypoints, the last one repeated
 *   nodes/gp_ad_mpc_node.py:344-349   resample_vel on the lane                           the clamp (clamp != 0)
 *   src/ad_mpc/ref_traj.py:67-86      RefTrajectory.set_traj on the lane                 serial cdist, unwrap, curvature   } admpc_waypoints_
 *   src/ad_mpc/ref_traj.py:10-25      compute_curvature, scipy's filtfilt                the 11-tap mean, both directions  } lane_batch
 *   src/ad_mpc/ref_traj.py:89-171     RefTrajectory.get_waypoints on the lane            the generator of admpc_waypoints_batch, M = L
 *   nodes/gp_ad_mpc_node.py:389-438 -> run_mpc :160-230   one pose message               admpc_control_step_lane_batch
 */
#ifndef ADMPC_LANE_H
#define ADMPC_LANE_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_fleet.h"      /* AdmpcPathBank: the bank of paths is the store of routes */

#ifdef __cplusplus
extern "C" {
#endif

/* L: waypoints of the lane, in [34, 256] (scipy's filtfilt refuses 33 samples or fewer; the lane is held in LDS).
 * back, ahead >= 0: the search window around the last answer, in waypoints. */
typedef struct AdmpcLaneParams { int32_t L, back, ahead; } AdmpcLaneParams;

/* The lane generator, one wavefront per vehicle.  Vehicle b is on route path_of[b] of the bank (M waypoints; only its vel, x, y and psi
 * columns are read).
 *   lane_idx [B] int32, device, in/out: where the vehicle's last lane began.  lane_idx[b] < 0: every waypoint of the route is searched
 *            for the nearest one; otherwise the window [max(0, i - back), min(M - 1, i + ahead)] with i = min(lane_idx[b], M - 1).
 *            Distance sqrt(dx^2 + dy^2), every operation rounded on its own; the first index of the minimum wins; where every distance
 *            is NaN (a non-finite pose) the first index of the searched range.  The result i0 is written back.  The window keeps a
 *            vehicle on its branch of a route that crosses itself, and the search O(window).
 *   the lane waypoints i0 .. i0 + L - 1 of the route; past the route's end the last waypoint is repeated (the node's padding rule,
 *            :372-376, extended from n_mpc_nodes to L).
 *   clamp    != 0: the node's resample_vel on the lane at the vehicle's speed, before anything else as in the node: bound =
 *            sqrt(vx^2 + vy^2); for i < L: vel[i] = vel[i] > bound ? bound : vel[i], bound += acc_max * clamp_dt * 0.8 (serial).
 *            admpc_resample_vel_batch is NOT to be run on the rows afterwards.
 *   set_traj serial cdist, numpy.unwrap of psi, compute_curvature = diff(unwrapped psi) / max(diff(cdist), 0.1) with the last value
 *            repeated, filtered by scipy's filtfilt(ones(11) / 11, 1, .): odd extension by 33 samples, the 11-tap mean forwards and
 *            backwards, the middle L samples.  A lane on which the reference's assert fires (an unwrapped yaw difference of exactly
 *            pi) is outside the contract.
 *   rows     get_waypoints on that table with M = L and the bank's H and dt: out_ref [B][6][H], out_err [B][3], out_stop [B] as for
 *            admpc_waypoints_batch (speeds padded with 0.01 where H > L).
 * A vehicle with path_of[b] outside [0, K) reads no route: NaN rows, out_stop[b] 0, lane_idx[b] untouched.
 * X_init, Y_init, psi_init, vx, vy [B] device.  No allocation, no host synchronisation, no workspace.
 * ADMPC_EINVAL: a null lane, L outside [34, 256], negative back / ahead, a null lane_idx (these four before anything else is looked
 * at), a null bank, B < 0, a null array; B == 0 is a no-op. */
int admpc_waypoints_lane_batch(const AdmpcPathBank* bank, const AdmpcLaneParams* lane, int B, const int32_t* path_of, int32_t* lane_idx,
                               const double* X_init, const double* Y_init, const double* psi_init,
                               const double* vx, const double* vy, int clamp, double acc_max, double clamp_dt,
                               double* out_ref, double* out_err, int32_t* out_stop, void* stream);

/* admpc_control_step_bank_batch (admpc_fleet.h) along a route: the lane generator takes the place of admpc_waypoints_bank_batch AND of
 * the clamp on the window behind it (prm->resample is the generator's `clamp`, prm->resample_dt its `clamp_dt`); the rest of the chain
 * -- assembly, admpc_solve_batch, the command kernel that masks `cost` -- is the bank step's, launch for launch.  The arrays, the
 * workspace (admpc_control_step_workspace), the refusals and the rule for a path_of[b] outside the bank (a failed solve for that
 * vehicle alone; its lane_idx stays) are the bank step's; the refusals of the lane parameters and of a null lane_idx come first.
 * No host synchronisation and no allocation once admpc_reserve(s, B) has run: the chain can be captured into a graph. */
int admpc_control_step_lane_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcLaneParams* lane, const AdmpcStepParams* prm, int B,
                                  const int32_t* path_of, int32_t* lane_idx,
                                  const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                                  const double* yaw_rate, const double* steer,
                                  double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid,
                                  void* work, float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_LANE_H */
