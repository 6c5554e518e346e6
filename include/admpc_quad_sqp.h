/*
 * admpc_quad_sqp.h -- solver_type "SQP" of the quadrotor MPC as ONE launch: the SQP loop of an instance inside the one-wave solve kernel
 * (libadmpc.so; csrc/admpc_quad.hip, admpc_quad_solve_kernel<P, true>).  The reference builds its point-tracking controllers with
 * {"solver_type": "SQP", "terminal_cost": True} (point_tracking_and_record.py:337-340, create_ros_gp_mpc.py:63-68).  A handle built with
 * cfg.sqp_iters > 1 serves that by a host loop of four launches per QP (admpc_quad.h), which no closed loop can afford and which every
 * rollout entry refuses.  The mode of this header is set on a handle built with sqp_iters <= 1, costs one launch per solve, and is flown
 * by every rollout entry as it stands.  An addition to admpc_quad.h, whose conventions hold here: device pointers owned by the caller,
 * dense; `stream` a hipStream_t passed as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message;
 * no host synchronisation and no allocation in a solve, which can be captured into a graph.
 *
 * THE LOOP of one instance (oracle/quad_oracle.c: quad_oracle_solve_batch with sqp_iters = qp_max, sqp_tol = tol):
 *   QP 0      shoot at the caller's iterate, condense, box QP, expansion, full step -- one SQP-RTI step of admpc_quad.h.
 *   QP q >= 1 shoot ONCE at the new iterate; with tol > 0 acados' stopping test on this linearisation, then the QP on the same one.
 *   the test  the inf-norms of the four KKT residuals of the NLP at the iterate, with the multipliers of the last QP (recovered by the
 *             adjoint recursion of its stationarity on its own linearisation): stationarity, shooting defects and x_0 - x0, violation of
 *             the input box, complementarity.  All four <= tol: status 0, the instance leaves.  A NaN in a norm never passes.
 *   a failed QP (a non-finite value, a matrix that is not positive definite): status 4 at once; the iterate is the one before that QP.
 *   qp_max QPs solved without passing the test: status 2 (ACADOS_MAXITER); the iterate is valid.
 *   tol == 0  no test: qp_max QPs, status 0 or 4 as for one step.
 * Every instance stops on its own; the wave then takes its next instance (from a work counter whenever the batch is larger than the grid).
 * The iterate stays in LDS between the QPs.  When the instance leaves: xbar / ubar its iterate, cost the last solved QP's, iters the
 * interior-point count of the last solved QP, status as above, qps the QPs started (acados' sqp_iter): q where the test passed in front
 * of QP q, q + 1 where QP q failed, qp_max at the limit.  The result is, bit for bit, that of a handle built with sqp_iters = qp_max,
 * sqp_tol = tol (tests/test_quad_sqp_gpu.py), and with tol == 0 that of qp_max single steps.
 *
 * DEVIATION from acados: no test precedes QP 0.  Every call starts cold -- it holds no multipliers -- so its first QP is always solved,
 * while acados keeps the multipliers of the previous call and may return after its test without solving one.  A closed loop therefore
 * pays at least one QP per period, and qps >= 1.
 *
 * IN A ROLLOUT (admpc_quad_fleet.h, _learn.h, _noise.h, _targets.h): the entries call admpc_quad_solve_batch_ex, which on a handle with
 * the mode on is this solve; admpc_quad_solver_info keeps reporting the configuration's sqp_iters, so they accept the handle.
 * counts[b][1] of a rollout counts the periods with a status other than 0: status 2 is counted as well as 4.
 *
 * NOT offered:
 *   - N > 16 (N nu > 64: the two-wave kernels; they keep the host loop of cfg.sqp_iters);
 *   - routed solves (admpc_quad_solve_batch_routed, clustered GP ensembles);
 *   - a line search or a step other than the full step (the reference's setting takes full steps);
 *   - multipliers kept between calls (the deviation above).
 *
 * Compiled for gfx950: no scratch, no spilled VGPR; LDS quad_lds_doubles(N) + 34 N + 13 doubles, 43 400 bytes at N = 10: three workgroups per CU.
 * The instantiations without the loop are unchanged.
 *
 * Measured on one MI355X, N = 10, (qp_max, tol) = (100, 1e-6), the forms alternating, medians of three (scripts/quad_sqp_time.py;
 * DESIGN.md section 7).  One solve, wall time with a synchronisation, the host loop of a handle built with sqp_iters = 100 against this
 * entry: B = 4096 (mean qps 61.9) 92.5 ms against 58.7 ms, B = 1 (33 QPs) 9.56 ms against 4.60 ms, the same bits.  rollout_targets at
 * B = 4096: a period 28.5 ms in SQP (mean qps 22.8; the vehicles at the limit set the time) against 0.718 ms in RTI; in 60 periods 3459
 * targets reached against 2574.
 */
#ifndef ADMPC_QUAD_SQP_H
#define ADMPC_QUAD_SQP_H

#include <stdint.h>
#include "admpc_quad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Turns the loop on (qp_max > 1) or off (qp_max <= 1) for a handle.  Host state that travels as kernel arguments: set it before a graph
 * capture, not between replays.  ADMPC_EINVAL, in this order: a null handle; qp_max outside [0, 10000]; tol NaN or negative; a handle
 * built with cfg.sqp_iters > 1 (that field keeps the launch-per-QP loop); qp_max > 1 on a handle with N nu > 64. */
int admpc_quad_set_sqp(AdmpcQuadSolver* s, int qp_max, double tol);

/* What admpc_quad_set_sqp left: qp_max (0: off) and tol; either pointer may be null. */
int admpc_quad_get_sqp(const AdmpcQuadSolver* s, int* qp_max, double* tol);

/* admpc_quad_solve_batch_ex with the loop above and qps [B] int32 (may be null, as cost, status and iters may).  ADMPC_EINVAL: a null
 * handle; a handle whose mode is off; then the refusals of admpc_quad_solve_batch_ex.  admpc_quad_solve_batch_ex (and admpc_quad_solve_batch)
 * on a handle with the mode on is this entry with qps = NULL. */
int admpc_quad_solve_batch_sqp(AdmpcQuadSolver* s, int B, const double* x0, const double* yref, const double* yref_e,
                               const double* gp_state, double* xbar, double* ubar, double* cost, int32_t* status,
                               int32_t* iters, int32_t* qps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_SQP_H */
