/*
 * admpc_quad_traj.h -- the reference trajectories of the quadrotor's experiments generated on the device (libadmpc.so;
 * csrc/admpc_quad_traj.hip): the loop and the lemniscate that ramp to v_max and back, with the attitude from the thrust direction, the
 * body rates from a numerical quaternion derivative under an accumulated yaw correction, and the feed-forward inputs from a second
 * numerical derivative.  A generated bank is an AdmpcQuadTrajBank of admpc_quad_fleet.h, the same object with the same layout (desc [K],
 * X [rows][13], U [rows][4] in one allocation): every entry that takes a bank takes a generated one.  An addition to admpc_quad_fleet.h,
 * whose conventions hold here: fp64; `stream` a hipStream_t passed as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error()
 * of admpc.h for the message; the caller's HIP device restored.  Every refusal listed below comes in front of the first device call, in
 * the order it is listed.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                replaced by
 *   --------------------------------------------------------------------------------------  ------------------------------------
 *   utils/trajectories.py:357-464   loop_trajectory (yawing=False, map_name=None)            } AdmpcQuadTrajSpec,
 *   utils/trajectories.py:467-561   lemniscate_trajectory (likewise)                         } admpc_quad_traj_bank_generate
 *   utils/trajectories.py:396-410   the five np.arange phases                                admpc_quad_traj_lengths
 *   utils/trajectories.py:128-282   minimum_snap_trajectory_generator, the branch `else` of  admpc_quad_traj_bank_generate
 *                                   `if yawing` and the branch `map_limits is None`
 *   experiments/trajectory_test.py:72-90, comparative_experiment.py  the trajectory a run flies   the generated bank
 *
 * DEVIATIONS, all deliberate: gravity is the literal 9.81 of trajectories.py:154 and NOT plant->g; `clockwise` is honoured for both
 * kinds (the reference's lemniscate ignores its flag: it is the clockwise one here); the yawing branch and the map limits are NOT
 * offered.  The reference's random_trajectory and straight_trajectory, piecewise polynomials through keyframes, are
 * admpc_quad_poly_traj.h's: their banks are this header's, and steps 4 .. 9 below and the passes B, C, D are theirs too (ONE text,
 * csrc/quad_traj_tail_dev.h).
 *
 * THE RULE.  For one trajectory let a = lin_acc / radius, M = n[0] + .. + n[4] its rows, i the row and j the row's index within its
 * phase.  t_total = 2 * v_max / lin_acc + 2 * 2, coasting = (t_total - 4 * 2) / 2, and the phases stop at 2, coasting, 4, coasting, 2:
 * n[p] = ceil(stop_p / dt), numpy's arange rule, evaluated in double.
 *   1. alpha: ramp  a * sin(pi / 4 * (j * dt))^2;  coast  a;  transition  a * cos(pi / 4 * (j * dt));  down-coast  -a;  last  ramp[j] - a;
 *      all negated where clockwise == 0.
 *   2. w = cumsum(alpha) * dt, angle = cumsum(w) * dt: both scans inclusive, the multiplication behind the scan.
 *   3. with s = sin(angle), c = cos(angle), R = radius:
 *        loop        pos (R s, R c, z)     vel (R w c, -R w s, 0)            acc (R (alpha c - w^2 s), -R (alpha s + w^2 c), 0)
 *        lemniscate  pos (R c, R s c, z)   vel (-R w s, R (w c^2 - w s^2), 0)
 *                    acc (-R (alpha s + w^2 c), R (alpha c^2 - 2 w^2 c s - alpha s^2 - 2 w^2 s c), 0)
 *   4. thrust = acc + (0, 0, 9.81), z_b = thrust / |thrust|, f_t = mass * (z_b . thrust), q = 0.5 * (1 + z_b.z, -z_b.y, z_b.x, 0),
 *      normalised.
 *   5. q_dot = np.gradient(q) / dt (central, (q[i+1] - q[i-1]) / 2; one-sided at both ends); w0[i] = 2 * (conj(q[i]) (x) q_dot[i])[1:4]
 *      with the product q_dot_q of utils.py:341.
 *   6. yaw[0] = 0, yaw[i] = sum over m = 1 .. i of (-w0[m].z * dt): a third inclusive scan, whose term of row 0 is 0;
 *      qn[0] = q[0], qn[i] = q[i] (x) (cos(yaw[i] / 2), 0, 0, sin(yaw[i] / 2)).
 *   7. qn_dot = gradient(qn) / dt; rate[0] = w0[0] (from the UNCORRECTED q[0], q[1]); rate[i] = 2 * (conj(qn[i]) (x) qn_dot[i])[1:4].
 *   8. rate_dot = gradient(rate) / dt; tau = rate_dot * J + ((J2 - J1) r2 r1, (J0 - J2) r0 r2, (J1 - J0) r1 r0);
 *      u = solve([y_f; -x_f; z_l_tau; 1 1 1 1], (tau, f_t)) / max_thrust.  The 4 x 4 matrix is inverted ONCE on the host (Gauss-Jordan
 *      with partial pivoting) and travels in the kernel's arguments.
 *   9. state row (pos, qn, vel, rate) with pos.x -= pos.x[0], pos.y -= pos.y[0].
 *
 * THE MAPPING.  One work-group of 256 lanes per trajectory (a grid cap and a stride loop over the trajectories); the rows are taken in
 * TILES of 256 consecutive rows, lane l of the group at row tile * 256 + l.  THE SCAN, the same text for all three:
 *   within a wave    the inclusive Hillis-Steele scan over its 64 lanes: for d = 1, 2, 4, 8, 16, 32: v[l] = v[l - d] + v[l] where l >= d
 *   across the waves wave m adds to every lane ((t_0 + t_1) + .. + t_(m-1)), the totals t of the waves in front of it, summed serially
 *                    from wave 0 (through LDS, one barrier); nothing for wave 0
 *   across the tiles the tile adds its carry-in to the sum of the two above: out = carry + (waves_before + v); the carry-out is `out` of
 *                    the tile's last lane; the carry into tile 0 is 0
 * A row past M - 1 contributes 0.  The per-lane serial run has length 1 (a lane holds one row of a tile); the serial part is the carry
 * from tile to tile.  The shape does not depend on K, on the place in the batch or on the grid; it does not even depend on M.
 * Four passes over the tiles of a trajectory, a barrier behind each tile and each pass (__syncthreads: the group's global writes and LDS
 * writes in front of it are visible to the group behind it):
 *   A  alpha, the two scans, steps 3 and 4: the rows (pos, q, vel, 0) and (0, 0, 0, f_t) staged in LDS and written by contiguous lanes
 *   B  w0 from q of rows i - 1, i, i + 1, the yaw scan: yaw[i] into U[i][0]
 *   C  qn of rows i - 1, i, i + 1 from q and yaw, rate[i] into X[i][10:13]
 *   D  rate_dot from the rates of rows i - 1, i, i + 1, u; the final rows (pos, qn, vel, rate) and u staged in LDS and written by
 *      contiguous lanes
 * Between the passes the intermediates live in the output rows themselves (q in X[.][3:7], f_t in U[.][3], yaw in U[.][0], the rate in
 * X[.][10:13]); a pass writes only what no other lane reads in that pass.  No atomics.
 */
#ifndef ADMPC_QUAD_TRAJ_H
#define ADMPC_QUAD_TRAJ_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_quad.h"
#include "admpc_quad_fleet.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_QUAD_TRAJ_MAX_M 16384   /* rows of one generated trajectory at most: a stated cap, the mapping needs none */

typedef struct AdmpcQuadTrajSpec {      /* one trajectory; 40 bytes */
    int32_t kind;        /* 0 loop (trajectories.py:357), 1 lemniscate (:467) */
    int32_t clockwise;   /* 0 / 1; 0 negates alpha (:425) -- the reference's lemniscate ignores the flag; here it is honoured for both kinds */
    double  radius, z, lin_acc, v_max;   /* all > 0, finite */
} AdmpcQuadTrajSpec;

/* The five phase lengths of a trajectory (above), on the HOST: no device is touched.
 * ADMPC_EINVAL, in this order: a null argument; kind outside {0, 1}; clockwise outside {0, 1}, or radius, z, lin_acc or v_max not
 * positive or not finite; dt not positive or not finite; an empty coasting phase, n[1] < 1 (v_max / lin_acc <= 2: the reference indexes
 * coasting_t_vec[-1] of an empty array there); M above ADMPC_QUAD_TRAJ_MAX_M. */
int admpc_quad_traj_lengths(double dt, const AdmpcQuadTrajSpec* spec, int32_t n[5]);

/* K trajectories generated into a new bank on `device`.  The lengths and offsets are computed on the host, the allocation and the
 * upload of the descriptors and the specs are synchronous (as admpc_quad_traj_bank_create is); the generation is enqueued on `stream`:
 * the bank is ready for work later on that stream, and after a stream synchronise for any other use.  specs [K] is a HOST pointer and is
 * not needed after the call (the kernel reads a device copy by pointer).  From `plant` mass, J, x_f, y_f, z_l_tau and max_thrust are
 * read; gravity is the literal 9.81, NOT plant->g.
 * ADMPC_EINVAL, in this order, each looked for in ALL K specs before the next: a null argument; K < 1; a kind outside {0, 1}; a
 * clockwise outside {0, 1}, or a radius, z, lin_acc or v_max not positive or not finite; dt not positive or not finite; an empty
 * coasting phase; an M above ADMPC_QUAD_TRAJ_MAX_M; then mass, an entry of J or max_thrust not positive (or not finite); an arm matrix
 * [y_f; -x_f; z_l_tau; 1] that is singular.  ADMPC_ENODEV, behind all of them: no such device. */
int admpc_quad_traj_bank_generate(int device, int K, const AdmpcQuadTrajSpec* specs, const AdmpcQuadPlantParams* plant, double dt,
                                  void* stream, AdmpcQuadTrajBank** bank);

/* What a bank holds, on the host: K, the rows of all trajectories, M [K] (each pointer but bank may be NULL).  ADMPC_EINVAL: a null bank. */
int admpc_quad_traj_bank_info(const AdmpcQuadTrajBank* bank, int* K, int64_t* rows, int32_t* M);

/* Trajectory k read back: traj_host [M_k][13], u_host [M_k][4] (HOST pointers, each may be NULL).  Synchronous: the device is
 * synchronised first.  ADMPC_EINVAL: a null bank; k outside [0, K). */
int admpc_quad_traj_bank_copy(const AdmpcQuadTrajBank* bank, int k, double* traj_host, double* u_host);

/* x[b] = state row idx[b] of trajectory traj_of[b], u[b] its input row (u: NULL or [B][4]), on `stream`; a vehicle whose traj_of or idx
 * is out of range gets NaN, the chunk kernel's rule.  One thread per double written.
 * ADMPC_EINVAL: a null bank; B < 0; then (B > 0) a null traj_of, idx or x.  B == 0 is a no-op. */
int admpc_quad_traj_rows_batch(const AdmpcQuadTrajBank* bank, int B, const int32_t* traj_of, const int32_t* idx, double* x, double* u,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_TRAJ_H */
