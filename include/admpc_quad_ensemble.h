/*
 * admpc_quad_ensemble.h -- a clustered GP ensemble in the quadrotor's closed loop, flown and learned on the device (libadmpc.so;
 * csrc/admpc_quad_ensemble.hip): one handle per cluster, the cluster of every vehicle taken from its reference window in every period,
 * and observe -> bin -> fit -> install per cluster.  An addition to admpc_quad.h, admpc_quad_fleet.h, admpc_quad_learn.h and
 * admpc_quad_noise.h, whose conventions hold here: device pointers owned by the caller, instance-major and dense, fp64; `stream` a
 * hipStream_t passed as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message; the caller's HIP
 * device restored; no host synchronisation and no allocation in the batch entries, which can be captured into a graph; every refusal in
 * front of the first device call, in the order it is listed; B == 0 and T == 0 are no-ops.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                  replaced by
 *   ----------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp_fitting.py     the recorded data cut into clusters in velocity space,     admpc_quad_ensemble_observe_batch: a record
 *                                   one GP per cluster and axis                                goes to the bins of ITS cluster;
 *                                                                                              admpc_quad_ensemble_fit
 *   quad_mpc/quad_3d_optimizer.py:207      one solver per cluster                              AdmpcQuadEnsemble: one handle per cluster
 *   quad_mpc/quad_3d_optimizer.py:485-491  set_reference_trajectory: the solver of a solve     admpc_quad_ensemble_route_batch, and every
 *                                   from the first row of the reference chunk                  period of admpc_quad_ensemble_rollout_batch
 *   model_fitting/gp.py:738-770     select_gp: the nearest centroid                            csrc/quad_route_dev.h, the body of
 *                                                                                              admpc_quad_select_cluster_kernel too
 *   quad_mpc/quad_3d_optimizer.py:289-327  where the GPs enter the model of the MPC            admpc_quad_ensemble_install
 *
 * NOT offered:
 *   - the GMM that finds the centroids (gp_fitting.py): to THESE entries the centroids are GIVEN; admpc_quad_clusters.h finds them from a
 *     log of the records flown, and installs them in the object's device copy;
 *   - the search of the hyperparameters by THESE entries: to admpc_quad_ensemble_fit the length scales, sigma_f and the noise of every
 *     cluster are GIVEN; admpc_quad_hyper.h searches them for all clusters in one chain of launches (admpc_quad_ensemble_search, _refit);
 *   - SQP mode (a handle with sqp_iters > 1 is refused: the rollout is the RTI loop).  The SQP loop inside the solve kernel of
 *     admpc_quad_sqp.h serves one-handle rollouts; routed solves refuse a handle that has it on.
 *
 * ONE ITERATE PER VEHICLE.  xbar / ubar of vehicle b are used by whichever cluster solves it: a vehicle that changes cluster is
 * warm-started from the other cluster's solution.  The reference keeps an iterate per solver instead (each acados solver its own), so
 * there a vehicle that returns to a cluster resumes from what that solver held when it last ran.
 *
 * ROUTING.  route[b] is the centroid nearest to the selected features of row 0 of vehicle b's window yref [B][N][17]: the first 13
 * entries are the reference state with its world-frame velocity, which is rotated into the body frame by that row's own quaternion; the
 * last 4 are the reference input.  Euclidean distance, ties to the lower index, a feature that is not finite gives route 0.  The
 * arithmetic is admpc_quad_select_cluster_kernel's, read through a row stride: one body (csrc/quad_route_dev.h), compiled as that kernel
 * always was, so on dense copies of row 0 admpc_quad_select_cluster_batch gives the same route bit for bit.  numpy gives it wherever the
 * two nearest distances differ by more than a few units in the last place.
 *
 * THE PARAMETER BLOCKS.  The K AdmpcQuadObserveParams are copied at create; their regressors reach the bin kernel from the object's
 * device copy (K * 3 regressors of 136 bytes each would come to within a quarter of the kernel-argument limit at K = 8), the centroids
 * likewise.  The observe kernel and the fit take their block from the host copy, as admpc_quad_learn.h's entries do.
 *
 * Measured on one MI355X at B = 4096, drag on, three regressors of 20 points in every handle, the forms alternating in one session,
 * medians of three (scripts/quad_ensemble_time.py), microseconds per closed-loop step at N = 10 / N = 20:
 * admpc_quad_rollout_batch 1163.3 / 2968.0; this rollout with K = 1 1168.5 / 2974.7 (5.2 / 6.7 more: the route kernel, 4.8 by trace, and
 * the route check of the routed solve, 4.9); with K = 4 on the body-frame v_x 3952.5 / 8420.9, which is 3.40 / 2.84 times the single
 * handle: every handle passes over the whole batch (a K = 4 step at N = 10 leaves about 970 for each handle's pass, against about 1090 for
 * the single handle that solves every instance; the launch geometry suggests why, without this having been measured apart: at most 2048 blocks take
 * two instances each at this size, and a block rarely finds neither to be its own).  Observed, K = 4: 97.5 / 64.6 more than unobserved (the single handle:
 * 46.5 / 47.9); by kernel trace admpc_quad_ensemble_bin_kernel 91.3 against admpc_quad_bin_kernel 41.8 (384 waves against 96, each walking
 * all 4096 records and routing every valid one).
 */
#ifndef ADMPC_QUAD_ENSEMBLE_H
#define ADMPC_QUAD_ENSEMBLE_H

#include <stdint.h>
#include "admpc.h"
#include "admpc_quad.h"
#include "admpc_quad_fleet.h"
#include "admpc_quad_learn.h"
#include "admpc_quad_noise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_QUAD_CLUSTERS_MAX 8

typedef struct AdmpcQuadEnsemble AdmpcQuadEnsemble;

/* K handles (owned by the caller, who keeps them alive as long as the object), n_feat features feats[] indexing
 * z = [x with the velocity in the body frame; u] (17 entries), HOST centroids [K][n_feat], and obs: NULL (an ensemble that only flies)
 * or K AdmpcQuadObserveParams, one per cluster (host; copied).  The object owns device copies of the centroids and of the regressors.
 * Synchronous.
 * ADMPC_EINVAL, in this order:
 *    1. a null solvers, feats, centroids or out; K outside 1 .. ADMPC_QUAD_CLUSTERS_MAX;
 *    2. a null handle;
 *    3. handles that do not share device and horizon;
 *    4. a handle with sqp_iters > 1;
 *    5. n_feat outside 1 .. 3, or a feature outside 0 .. 16;
 *    6. a centroid that is not finite;
 *   and with obs:
 *    7. each block, in the order of the clusters, as admpc_quad_learn.h refuses an AdmpcQuadObserveParams;
 *    8. blocks that differ in dt, substeps, n_gp, or in a regressor's n_feat, feat or out (the box, nb and the hyperparameters may
 *       differ per cluster: that freedom is the point of the per-cluster blocks);
 *    9. a clustering feature outside 7 .. 16: the sample record holds only those entries;
 *   10. a handle whose n_gp is not the blocks' n_gp (create it with placeholder GPs of n_points = 0). */
int admpc_quad_ensemble_create(AdmpcQuadSolver* const* solvers, int K, int n_feat, const int32_t* feats, const double* centroids,
                               const AdmpcQuadObserveParams* obs, AdmpcQuadEnsemble** out);
void admpc_quad_ensemble_destroy(AdmpcQuadEnsemble* e);

/* route [B] int32 <- the cluster of every vehicle from row 0 of its window yref [B][N][17], N the handles' horizon (ROUTING above).
 * One thread per vehicle.  ADMPC_EINVAL, in this order: a null ensemble; B < 0; then (B > 0) a null array. */
int admpc_quad_ensemble_route_batch(const AdmpcQuadEnsemble* e, int B, const double* yref, int32_t* route, void* stream);

/* admpc_quad_observe_batch of admpc_quad_learn.h for the ensemble.  Two launches.
 *   1. admpc_quad_observe_kernel, unchanged: samples [B][14] as admpc_quad_learn.h lays them out, under dt and substeps of the blocks
 *      (they share them).
 *   2. admpc_quad_ensemble_bin_kernel, one wave per (cluster c, regressor g, bin), all clusters in ONE launch.  The wave computes the
 *      cluster of each valid record itself: the centroid nearest to the record's own features, feature f reading entry f - 7, by the
 *      distance arithmetic of the routing above.  A valid record of another cluster is absent to the wave: not added, not counted as
 *      dropped.  Everything else is the contract of admpc_quad_bin_kernel with cluster c's box (one body, csrc/gp_fit_dev.h): lane l adds
 *      b = l, l + 64, ... into its own partial sum from 0 -- a record keeps its lane whether or not the cluster takes it -- and the 64
 *      partial sums then go onto the stored value one after the other, lane 0 first.
 *      bins [K][3][32][5], in/out.  dropped [K][4] int32, in/out: [c][g] grows by the valid records of cluster c outside regressor g's
 *      box, [0][3] by the records that are not valid; [c > 0][3] stay as given.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; the plant parameters as
 * admpc_quad_plant_step_batch refuses them; a null model; B < 0; then (B > 0) a null array; u_stride < 4. */
int admpc_quad_ensemble_observe_batch(const AdmpcQuadEnsemble* e, const AdmpcQuadSolver* model, const AdmpcQuadPlantParams* plant, int B,
                                      const double* u, int64_t u_stride, const double* x, double* prev, double* samples, double* bins,
                                      int32_t* dropped, void* stream);

/* bins [K][3][32][5] -> gp_out [K][3] AdmpcGp records in device memory and info [K][3] int32: cluster c is admpc_quad_gp_fit of bins[c]
 * under block c, in every respect (K launches of the fit kernel); the entries of a regressor past n_gp are not written.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; min_count < 1; a null array. */
int admpc_quad_ensemble_fit(const AdmpcQuadEnsemble* e, int min_count, const double* bins, AdmpcGp* gp_out, int32_t* info, void* stream);

/* gp_dev [K][3] into the K handles, installed [K][3] int32: cluster c is admpc_quad_gp_install(solvers[c], n_gp, gp_dev[c],
 * installed[c]) with the n_gp handle c was created with.  A record the check refuses becomes the empty GP in its cluster only.  A captured
 * graph that flies the ensemble reads the new GPs at its next replay.
 * ADMPC_EINVAL, in this order: a null ensemble; a handle created without GPs; a null array. */
int admpc_quad_ensemble_install(AdmpcQuadEnsemble* e, const AdmpcGp* gp_dev, int32_t* installed, void* stream);

/* admpc_quad_rollout_noise_batch (admpc_quad_noise.h) with the ensemble in place of the solver: T closed-loop steps, each
 *   window (admpc_quad_ref_chunk_batch's launch) -> routing from the window -> admpc_quad_solve_batch_routed -> plant
 * and, with the watch block, the two launches of admpc_quad_ensemble_observe_batch behind the plant (one latch of x in front of the
 * first step).  The arguments up to u_out are admpc_quad_rollout_batch's.
 *   route      [B] int32: the clusters of the LAST period on return
 *   route_out  NULL or [T][B] int32: the clusters of every period
 *   model, prev, samples, bins, dropped: the watch block of admpc_quad_rollout_observe_batch without its obs, which the object holds;
 *              model == NULL: not observed, and the four behind it are not read
 *   noise, noise_step: the disturbances of admpc_quad_rollout_noise_batch; noise == NULL: the deterministic plant, noise_step not read
 * ADMPC_EINVAL, in this order: a null ensemble; a model with an ensemble created without observe parameters; with noise, the plant
 * parameters and the disturbances as admpc_quad_rollout_noise_batch refuses them; then every refusal of the entry it extends
 * (admpc_quad_rollout_observe_batch with a model, admpc_quad_rollout_batch without), in that entry's order and under that entry's name,
 * a null route among its arrays; a null noise_step. */
int admpc_quad_ensemble_rollout_batch(AdmpcQuadEnsemble* e, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over,
                                      int B, int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                      double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                      double* tally, int32_t* counts, double* traj_out, double* u_out,
                                      int32_t* route, int32_t* route_out,
                                      const AdmpcQuadSolver* model, double* prev, double* samples, double* bins, int32_t* dropped,
                                      const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_ENSEMBLE_H */
