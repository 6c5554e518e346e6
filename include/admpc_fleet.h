/*
 * admpc_fleet.h -- the fleet step against a BANK of paths, and the arg-min per group of candidates (libadmpc.so; csrc/admpc_step.hip,
 * csrc/admpc_kernels.hip).  An addition to admpc.h, whose conventions hold here: device pointers owned by the caller, `stream` a
 * hipStream_t passed as void*, 0 or a negative ADMPC_E* code returned, admpc_last_error() for the message.
 *
 * admpc_control_step_batch (admpc.h) serves B vehicles on ONE global path and throws the objective of each solve away.  The entry points
 * below let every vehicle of a launch follow a path of its own, return the objective, and reduce it per group of consecutive
 * instances -- so that V vehicles x C candidate paths are one step (instance b = v * C + c) and one arg-min (G = V, group = C):
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/ad_mpc/...)                  replaced by
 *   -------------------------------------------------------------------------------  ------------------------------------
 *   ref_traj.py:67-86     RefTrajectory.set_traj, one object per route               admpc_path_bank_create (K routes, one allocation)
 *   ref_traj.py:89-171    RefTrajectory.get_waypoints                                admpc_waypoints_bank_batch
 *   gp_ad_mpc_node.py:389-438 -> run_mpc :160-230   one pose message                 admpc_control_step_bank_batch
 *   (new capability, BASELINE.json north_star)  arg-min over candidate costs          admpc_argmin_groups
 */
#ifndef ADMPC_FLEET_H
#define ADMPC_FLEET_H

#include <stdint.h>
#include "admpc.h"      /* AdmpcSolver, AdmpcPath, AdmpcStepParams, ADMPC_* codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct AdmpcPathBank AdmpcPathBank;   /* opaque */

/* A bank of K global paths on HIP device `device`.  `paths` is a HOST array of K descriptors whose seven columns are device arrays
 * [M] as for admpc_waypoints_batch (built by RefTrajectory.set_traj, ref_traj.py:67-86, plus the unwrapped yaw).  The bank copies every
 * column into ONE allocation of its own and keeps a device table of K descriptors (M and the offset of each column) next to them; the
 * caller may free its arrays afterwards.  Creation allocates and synchronises; nothing that takes a bank afterwards does.
 * ADMPC_EINVAL: K < 1, a path with M < 2 or a null column, paths that differ in H or dt, H outside [3, 64] (the waypoint kernel's
 * horizon), dt <= 0.  ADMPC_ENODEV: no such device. */
int  admpc_path_bank_create(int device, int K, const AdmpcPath* paths, AdmpcPathBank** out);
void admpc_path_bank_destroy(AdmpcPathBank* bank);

/* admpc_waypoints_batch (ref_traj.py:89-171) with a path per vehicle: pose b is laid against path path_of[b] of the bank -- the same
 * kernel text with another path lookup, so the rows of a vehicle are bit for bit those of admpc_waypoints_batch called with its path
 * alone (nearest waypoint with the first-index tie rule and index 0 for a non-finite pose, the serial running sums with the first H
 * path speeds padded with 0.01 when M < H, numpy.interp, the unwrap, the three-point splice).
 *   path_of  [B] int32, device.  A vehicle with path_of[b] outside [0, K) reads no path: its rows of out_ref and out_err are NaN and
 *            out_stop[b] is 0.
 *   X_init, Y_init, psi_init [B]; out_ref [B][6][H], out_err [B][3], out_stop [B] as for admpc_waypoints_batch (H and dt: the bank's). */
int admpc_waypoints_bank_batch(const AdmpcPathBank* bank, int B, const int32_t* path_of,
                               const double* X_init, const double* Y_init, const double* psi_init,
                               double* out_ref, double* out_err, int32_t* out_stop, void* stream);

/* admpc_control_step_batch (gp_ad_mpc_node.py:389-438 -> run_mpc :160-230) with a path per vehicle and the objective of each solve.
 * The chain, the arrays, the workspace (admpc_control_step_workspace) and the refusals are those of admpc_control_step_batch, with the
 * bank's H in place of the path's: waypoints (admpc_waypoints_bank_batch) -> speed clamp -> assembly -> admpc_solve_batch -> command.  A
 * vehicle on path k ends the step bit for bit as admpc_control_step_batch on path k alone would end it.
 *   path_of [B] int32, device.  A vehicle with path_of[b] outside [0, K) ends the step as a vehicle whose solve failed: its NaN
 *           reference rows make the solve report status 4 and leave the iterate alone, so safe_count is reset, the record is the brake
 *           record, valid is 0, prev_u and has_valid keep their values and cost is +inf.  Its neighbours are not affected.
 *   cost    [B] (may be NULL): the objective admpc_solve_batch returns for the vehicle, and +inf wherever status[b] != 0 or
 *           valid[b] == 0 (is_valid_command against the padded target, ad_3d_optimizer.py:466), so that admpc_argmin_groups picks among
 *           usable candidates only.  NOTE the difference from cost_io of admpc_actuation_batch, which is masked by mode == 0: mode also
 *           carries the safe_count gate (gp_ad_mpc_node.py:206-213), a warm-up of `threshold` steps per slot during which every mode is
 *           0; candidates have to be comparable during the warm-up, so the mask here does not use mode.
 * No host synchronisation and no allocation once admpc_reserve(s, B) has run: the chain can be captured into a graph. */
int admpc_control_step_bank_batch(AdmpcSolver* s, const AdmpcPathBank* bank, const AdmpcStepParams* prm, int B, const int32_t* path_of,
                                  const double* px, const double* py, const double* yaw, const double* vx, const double* vy,
                                  const double* yaw_rate, const double* steer,
                                  double* xbar, double* ubar, int32_t* safe_count, double* prev_u, int32_t* has_valid,
                                  void* work, float* ack, int32_t* mode, int32_t* valid, int32_t* status, double* cost, void* stream);

/* admpc_argmin per group of `group` consecutive costs: group g is cost[g * group .. (g + 1) * group); val[g] is its smallest cost and
 * idx[g] the index of that cost in the BATCH (not in the group).  The rules are admpc_argmin's (csrc/argmin_rule.h) with the group's
 * offset applied: a NaN cost is read as +inf and never beats a finite one, ties go to the lower index, a group with nothing finite
 * gives (+inf, its first index).  One wavefront per group; groups of up to 16 costs are packed four to a wavefront.
 * cost [G * group], val [G], idx [G]: device arrays.  ADMPC_EINVAL: G < 0, group < 1, G * group beyond INT32_MAX, a null array;
 * G == 0 is a no-op. */
int admpc_argmin_groups(AdmpcSolver* s, const double* cost, int G, int group, double* val, int64_t* idx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_FLEET_H */
