/*
 * admpc_quad_poly_traj.h -- reference trajectories through keyframes generated on the device (libadmpc.so;
 * csrc/admpc_quad_poly_traj.hip): the piecewise degree-7 polynomial that the reference fits through n_key position keyframes, sampled
 * with its first two derivatives and fed into the generator of admpc_quad_traj.h (attitude from the thrust direction, body rates under
 * the accumulated yaw correction, feed-forward inputs).  This is the reference's random_trajectory (10 keyframes of a sampled Gaussian
 * process, the first trajectory type of its comparative experiment) and its straight_trajectory (3 keyframes); the keyframes themselves
 * are made on the host (30 doubles per trajectory).  A generated bank is an AdmpcQuadTrajBank, the same object a loop bank or an
 * uploaded bank is: every entry that takes a bank takes it (admpc_quad_traj_bank_info, _copy, _rows_batch, _destroy, the window, the
 * rollouts).  An addition to admpc_quad_traj.h, whose conventions hold here: fp64; `stream` a hipStream_t passed as void*; 0 or a
 * negative ADMPC_E* code returned, admpc_last_error() for the message; the caller's HIP device restored.  Every refusal listed below
 * comes in front of the first device call, in the order it is listed.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                replaced by
 *   --------------------------------------------------------------------------------------  ------------------------------------
 *   utils/trajectories.py:307-321   straight_trajectory                                      } keyframes of the caller,
 *   utils/trajectories.py:324-354   random_trajectory (map_name=None), behind its keyframes  } admpc_quad_poly_traj_bank_generate
 *   utils/trajectories.py:314-315, 341-342; trajectory_generator.py:97-99                    admpc_quad_poly_traj_lengths
 *   utils/trajectory_generator.py:147-213, 255-265  fit_multi_segment_polynomial_trajectory, admpc_quad_poly_traj_weights (the matrix
 *                                   multiple_waypoints, matrix_generation, rhs_generation    once per call, on the host), step 1
 *   utils/trajectory_generator.py:91-144   get_full_traj (a float target_dt)                 steps 2 and 3 (pass A')
 *   utils/trajectories.py:128-282   minimum_snap_trajectory_generator, the branch `else` of  steps 4 .. 9 of admpc_quad_traj.h: its
 *                                   `if yawing` and the branch `map_limits is None`          passes B, C, D, the same text
 *   experiments/comparative_experiment.py:245  traj_type_vec[0] = {"random": 1}              the generated bank
 *
 * NOT offered: map limits (apply_map_limits, the `else` of map_limits is None) and the yawing branch.  The keyframes' attitude is
 * identically zero in the reference (keyframe_3d_gen.py:111-113 multiplies by 0), so its yaw polynomial is zero, `yawing` is False and
 * the fourth fitted dimension is not computed here; the jerk (der_order 3) is computed there and never read in the non-yawing branch.
 *
 * THE RULE.  n_seg = n_key - 1 segments; p [n_key][3] the keyframes of one trajectory.
 *   0. lengths, in double: d_m = sqrt((dx^2 + dy^2) + dz^2) of keyframes m and m + 1, av_dist = their mean (numpy's pairwise sum),
 *      av_dt = av_dist / speed, s = round-half-even(av_dt / dt), T = s * dt (one product), M = n_seg * s + 1.
 *      Why M: the reference's t_vec = np.arange(0, T * (n_seg + 1) - 1e-5, T) has n_seg + 1 entries seg * T, and each segment's
 *      np.arange(t0, t_next + 1e-5, dt) has ceil((t_next + 1e-5 - t0) / dt) entries.  (t_next - t0) / dt is s up to a relative error of
 *      (2 n_seg + 3) u < 1e-14, an absolute one below 1e-14 * s <= 1.7e-10 with s <= 16384; 1e-5 / dt lies in [1e-8, 1e-2] for dt in
 *      [1e-3, 1e3], so the quotient lies strictly between s and s + 1 and the count is s + 1.  All but the last segment drop their last
 *      sample: n_seg * s + 1 rows.  For dt above 1e3 the count is taken by the same formula (a deviation: nothing flies at such a dt).
 *   1. coefficients: the reference solves M_fit c = S p per axis, M_fit = multiple_waypoints(n_seg) of size 8 n_seg, S the scatter of
 *      rhs_generation.  Here c = W p with W = M_fit^-1 S, [8 n_seg][n_key], the same for every trajectory of that key count: computed once
 *      per call on the HOST by Gauss-Jordan elimination with partial pivoting in long double, rounded to double, uploaded next to the
 *      descriptors.  c[seg][a][axis] = sum over m = 0 .. n_key - 1, in index order, of W[8 seg + a][m] * p[m][axis]; a is the power
 *      of the monomial (ascending, as the reference's unknowns; its fliplr makes them descending for np.polyval).
 *   2. row i: seg = i / s and j = i - seg * s; the last row, i = n_seg * s, belongs to the last segment with j = s.
 *      t0 = seg * T, t_next = (seg + 1) * T, t1 = ((t0 + j * dt) - t0) / (t_next - t0) * 2 - 1, compress = 2 / (t_next - t0): every
 *      operation rounded by itself (no fused multiply-add).
 *   3. for k = 0, 1, 2 (position, velocity, acceleration) and each axis: the coefficients of np.polyder, highest power first,
 *      ((c_7 * 7) * 6) .. for k = 2, (c_7 * 7) .. for k = 1, each product rounded; np.polyval's Horner y = y * t1 + coefficient from the
 *      highest, each operation rounded by itself; times compress^k (1, compress, compress * compress).
 *   4. step 4 of admpc_quad_traj.h with acc from step 3: thrust = acc + (0, 0, 9.81), z_b = thrust / |thrust|,
 *      f_t = mass * (z_b . thrust), q = 0.5 * (1 + z_b.z, -z_b.y, z_b.x, 0), normalised.  A thrust that vanishes (acc.z = -9.81) is NOT
 *      refused: the rows come out non-finite, as the reference's do.
 *   5 .. 9. steps 5 .. 9 of admpc_quad_traj.h.
 *
 * THE MAPPING.  One work-group of 256 lanes per trajectory, a grid cap of 512 groups and a stride loop over the trajectories, tiles of
 * 256 consecutive rows: admpc_quad_traj.h's.  Per trajectory:
 *   coefficients  the 8 n_seg * 3 dot products of step 1, one per lane in a stride loop, into LDS (at most 5952 bytes); a barrier
 *   A'            steps 2 .. 4 for lane l's row tile * 256 + l, the coefficients of its segment read from LDS; the rows (pos, q, vel, 0)
 *                 and (0, 0, 0, f_t) staged in LDS and written by contiguous lanes; a barrier behind the staging and behind the writes
 *   B, C, D       csrc/quad_traj_tail_dev.h, the text the loop generator runs
 * No scan in A' (a row depends on its own index alone), no atomics; the bits of a trajectory do not depend on K, on its place in the
 * batch or on the grid.
 */
#ifndef ADMPC_QUAD_POLY_TRAJ_H
#define ADMPC_QUAD_POLY_TRAJ_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_quad.h"
#include "admpc_quad_fleet.h"
#include "admpc_quad_traj.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_QUAD_POLY_TRAJ_MIN_KEYS 3    /* the reference's matrix builder fails at 2 */
#define ADMPC_QUAD_POLY_TRAJ_MAX_KEYS 32   /* a stated cap: the coefficients of a trajectory stay below 6 KB of LDS */
#define ADMPC_QUAD_POLY_TRAJ_MIN_DT 1e-3   /* below it the reference's 1e-5 of np.arange stops deciding the row count (THE RULE, 0) */

/* s and M of one trajectory (THE RULE, 0), on the HOST: no device is touched.  keys [n_key][3], row-major.
 * ADMPC_EINVAL, in this order: a null argument; n_key outside [3, 32]; a keyframe coordinate that is not finite; speed or dt not positive
 * or not finite; dt below 1e-3; s < 1; M above ADMPC_QUAD_TRAJ_MAX_M.  A refused call writes nothing. */
int admpc_quad_poly_traj_lengths(double dt, int n_key, const double* keys, double speed, int32_t* s, int32_t* M);

/* W = M_fit^-1 S of THE RULE, 1, as the generator computes it: W [8 (n_key - 1)][n_key], row-major, on the HOST.
 * ADMPC_EINVAL, in this order: a null argument; n_key outside [3, 32]. */
int admpc_quad_poly_traj_weights(int n_key, double* W);

/* K trajectories through n_key keyframes each, generated into a new bank on `device`.  keys_host [K][n_key][3] and speed_host [K] are
 * HOST pointers and are not needed after the call.  The lengths, the offsets and W are computed on the host, the allocation and the
 * uploads are synchronous (as admpc_quad_traj_bank_generate's are); the generation is enqueued on `stream`: the bank is ready for work
 * later on that stream, and after a stream synchronise for any other use.  From `plant` mass, J, x_f, y_f, z_l_tau and max_thrust are
 * read; gravity is the literal 9.81, NOT plant->g.
 * ADMPC_EINVAL, in this order, each looked for in ALL K trajectories before the next: a null argument; K < 1; n_key outside [3, 32]; a
 * keyframe coordinate that is not finite; a speed, then dt, not positive or not finite; dt below 1e-3; an s < 1; an M above
 * ADMPC_QUAD_TRAJ_MAX_M; then the plant's refusals of admpc_quad_traj_bank_generate (mass, an entry of J or max_thrust not positive or
 * not finite; a singular arm matrix).  ADMPC_ENODEV, behind all of them: no such device. */
int admpc_quad_poly_traj_bank_generate(int device, int K, int n_key, const double* keys_host, const double* speed_host,
                                       const AdmpcQuadPlantParams* plant, double dt, void* stream, AdmpcQuadTrajBank** bank);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_POLY_TRAJ_H */
