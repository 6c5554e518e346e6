/*
 * admpc_quad_clusters.h -- the first stage of the training of a clustered GP ensemble, on the device (libadmpc.so;
 * csrc/admpc_quad_clusters.hip): a log of the sample records a fleet flies, a Gaussian-mixture EM that turns the log into centroids, an
 * install that the routing and the bin kernel pick up on the stream, and a re-bin of the log under the new centroids.  With it
 * record -> cluster -> fit -> install is one chain of launches on one stream.  An addition to admpc_quad_ensemble.h, whose conventions
 * hold here: device pointers owned by the caller, dense, fp64; `stream` a hipStream_t passed as void*; 0 or a negative ADMPC_E* code
 * returned, admpc_last_error() of admpc.h for the message; the caller's HIP device restored; no host synchronisation and no allocation in
 * any entry, each of which can be captured into a graph; every refusal in front of the first device call, in the order it is listed; an
 * empty batch (B == 0, T == 0, M == 0, steps == 0) is a no-op.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                  replaced by
 *   ----------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp_fitting.py:190   the recorded flight read back for the clustering         admpc_quad_ensemble_rollout_log_batch: the
 *                                                                                              records of every step stay on the device
 *   model_fitting/gp_common.py:224-271  GaussianMixture(n_clusters).fit(x_pruned), gmm.means_   admpc_quad_clusters_fit: sklearn's EM for
 *                                     the centroids                                            full covariances from GIVEN initial means
 *   model_fitting/gp.py:592-596       the clusters of a loaded ensemble sorted along the       admpc_quad_clusters_install: the means into
 *                                     first feature                                            the ensemble's device centroids, sorted
 *   model_fitting/gp_common.py:224-271  the records split by cluster, one GP per cluster        admpc_quad_clusters_rebin, then
 *                                                                                              admpc_quad_ensemble_fit / _install
 *
 * NOT offered:
 *   - k-means++ and random initialisation, n_init restarts, by THESE entries: the start is the given means (init, or the ensemble's present
 *     centroids); admpc_quad_kmeans.h has scikit-learn's k-means++ seeding, its Lloyd k-means and the n_init rule in front of this fit;
 *   - covariance types other than "full"; choosing K: K is the ensemble's;
 *   - the soft top-2 membership of gp_common.py:253-262: a record trains only its nearest cluster, as admpc_quad_ensemble.h bins it;
 *   - the PCA point selection of gp_fitting.py:237-240;
 *   - the search of the hyperparameters by THESE entries: admpc_quad_hyper.h has it, for all clusters at once, and after an install of new
 *     centroids and a re-bin it is what finds each cluster's length scales from the data the cluster holds now; SQP mode
 *     (admpc_quad_ensemble.h).
 *
 * CLUSTER c KEEPS BLOCK c.  The install moves centroids only: cluster c, the c-th along the first feature, goes on binning under the box
 * and fitting at the hyperparameters of the c-th AdmpcQuadObserveParams the ensemble was created with, and flies handle c.
 *
 * THE RECORDS are admpc_quad_learn.h's [14]: clustering feature f (7 .. 16) reads entry f - 7, entry 13 is the validity flag.  A record
 * counts in the fit if its flag is 1.0 and its d = n_feat clustering features are finite; n_valid is their number.
 *
 * THE STATE.  gmm [1 + K][ADMPC_GMM_ROW] doubles.  Row 0: the lower bound (the mean over the valid records of the log-likelihood under the
 * parameters the last E step read; -inf after the start), the last change of it (+inf after the start), n_valid; the rest is not used.
 * Row 1 + k, component k:
 *   [0]        weight w_k
 *   [1 .. 3]   mean, the features past d at 0
 *   [4 .. 9]   covariance, upper triangle by rows (00 01 02 11 12 22); the features past d carry the identity's rows
 *   [10 .. 15] P_k, the upper-triangular Cholesky factor of the precision (sklearn's precisions_cholesky_), same order
 *   [16]       the sum of log P_k,jj
 *   [17]       N_k
 * info [4] int32: iterations done, converged, status, n_valid.  status: 0; -(k + 1) if component k (the lowest such) had a Cholesky pivot
 * that is not positive and finite; ADMPC_GMM_ENOVALID if no record is valid.  A failure leaves gmm and the iteration count as the
 * iteration before it left them (a failed start: as the caller gave them) and stops the iterations behind it.
 *
 * DETERMINISM.  No floating-point atomics.  The grid of the E kernel is min(ceil(M / 256), ADMPC_GMM_BLOCKS_MAX) blocks of 256 threads, a
 * function of M alone; every block writes one row of `partial`, and one wave adds the rows in a fixed order.  Two runs on the same input
 * give the same bits.  The order inside the sums is not part of the contract.
 *
 * Measured on one MI355X at B = 4096, 60 logged steps (M = 245 760 records), K = 4, N = 10, on d = 1 (the body-frame v_x) / d = 3 (the
 * body-frame velocity), captured graphs replayed, both routes in one session, medians of three (scripts/quad_clusters_time.py; DESIGN
 * section 7), microseconds: one EM iteration 25.0 / 25.0 (by kernel trace the E kernel 15.9, the M kernel 9.6; a launch that returns at
 * once 2 to 4); pack and start 36.3 / 37.5 (the pack kernel 6.7 by trace); the whole chain of a fleet's fit_clusters() -- the fit at
 * sklearn's defaults, of whose 100 iterations 14 ran, the install, the bins zeroed, the re-bin -- 6543 / 8602, of which the re-bin's 60
 * launches of the bin kernel are 5902 / 7962.  The route it replaces -- the log to the host 2214 / 701, sklearn from the same start
 * 480 880 / 790 792 (14 iterations too), the centroids uploaded and a re-flight's worth of binning 6295 / 8363 -- 489 389 / 799 856: 75 /
 * 93 times as long.  An iteration reads 7.9 MB, far below what the memory system delivers in 25 microseconds: fewer than four records per
 * thread, and the latencies of a block (flags, component blocks, records, 41 wave reductions) one after the other.
 */
#ifndef ADMPC_QUAD_CLUSTERS_H
#define ADMPC_QUAD_CLUSTERS_H

#include <stdint.h>
#include "admpc_quad_ensemble.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_GMM_BLOCKS_MAX 256
#define ADMPC_GMM_ROW 18
#define ADMPC_GMM_PARTIAL 81            /* doubles per row of `partial`: 10 per component (sum r, r D [3], r D D' [6]) for 8, and the log-likelihood */
#define ADMPC_GMM_ENOVALID (-100)

/* admpc_quad_ensemble_rollout_batch, observed, with the records of step t written to log[t] ([T][B][14]) and binned from there; `samples`
 * is neither read nor written (it may be NULL).  In every other respect that entry: the arguments are its own, then log.
 * ADMPC_EINVAL, in this order: what admpc_quad_ensemble_rollout_batch refuses, under that entry's rules -- with a null model those of the
 * unobserved rollout up to its arrays, with a model every refusal of the observed one -- ; a null model (logging implies observing); then
 * (B > 0 and T > 0) a null log. */
int admpc_quad_ensemble_rollout_log_batch(AdmpcQuadEnsemble* e, const AdmpcQuadTrajBank* bank, const AdmpcQuadPlantParams* plant, int over,
                                          int B, int T, const int32_t* traj_of, int32_t* idx, double* x, double* xbar, double* ubar,
                                          double* yref, double* yref_e, double* cost, int32_t* status, int32_t* iters,
                                          double* tally, int32_t* counts, double* traj_out, double* u_out,
                                          int32_t* route, int32_t* route_out,
                                          const AdmpcQuadSolver* model, double* prev, double* samples, double* bins, int32_t* dropped,
                                          const AdmpcQuadNoiseParams* noise, uint64_t* noise_step, double* log, void* stream);

/* records [M][14] -> gmm, info (THE STATE above): sklearn.mixture.GaussianMixture(K, covariance_type="full") from given means, K, d and
 * the features the ensemble's.  1 + 2 (resume == 0) + 2 * max_iter launches, whatever the data:
 *   pack   one thread per record: packed[i] = (z_0, z_1, z_2, flag), the features past d at 0, flag 1.0 for a record that counts and 0.0
 *          otherwise.  The EM reads these 32 bytes per record and iteration, not the record's 112.
 *   start  (resume == 0) hard responsibilities -- a record belongs to the nearest initial mean, by the body routing and the bin kernel use
 *          (csrc/quad_route_dev.h; ties to the lower index) -- and one M step from them.  init: device [K][d], or NULL for the ensemble's
 *          present device centroids.  Sets iterations = 0, converged = 0, the lower bound -inf.
 *   E      per valid record and component, sklearn's full-covariance form
 *              log p_k = log w_k + sum_j log P_k,jj - d/2 log 2 pi - 1/2 |(x - mu_k)' P_k|^2,
 *          the log-sum-exp over k and the responsibilities r_k; every block writes its sums of r_k, r_k D and r_k D D' with
 *          D = x - mu_k about the CURRENT mean, and of the log-sum-exp, as one row of partial.
 *   M      one wave: adds the rows, then N_k = sum r_k + 10 * 2^-52, w_k = N_k / n_valid, s = sum r_k D / N_k, mu_k <- mu_k + s,
 *          Sigma_k = sum r_k D D' / N_k - s s' + reg_covar I, its Cholesky factor, P_k and the log-diagonal; the lower bound, its change
 *          from the one before, iterations + 1, and converged if |change| < tol.  (The moments are shifted because the one-pass
 *          sum r x x' - N mu mu' cancels.)
 * Once converged or a status is set, the kernels of the remaining iterations read the flag and return at once.  resume == 1 initialises
 * nothing and goes on from gmm and info as they stand: R calls of one iteration give, bit for bit, what one call of R iterations gives.
 * packed [M][4] and partial [ADMPC_GMM_BLOCKS_MAX][ADMPC_GMM_PARTIAL] are scratch of the caller's.
 * ADMPC_EINVAL, in this order: a null ensemble; a clustering feature outside 7 .. 16 (the record holds no others); max_iter outside
 * 1 .. 1000; a tol that is negative or NaN; a reg_covar that is negative or not finite; a resume other than 0 and 1; M < 0; then (M > 0)
 * a null records, packed, partial, gmm or info. */
int admpc_quad_clusters_fit(const AdmpcQuadEnsemble* e, int max_iter, double tol, double reg_covar, int resume, int64_t M,
                            const double* records, const double* init, double* packed, double* partial, double* gmm, int32_t* info,
                            void* stream);

/* One wave.  If info's status is 0 and every mean of gmm is finite: the means into the ensemble's device centroids, sorted ascending by
 * the first feature, ties to the lower component; perm [K] int32: perm[c] is the component that became cluster c; installed [1] int32 = 1.
 * Otherwise the centroids stay, perm is the identity and installed = 0.  The route kernel and the bin kernel take the centroids by
 * pointer: a captured rollout flies the new clusters at its next replay.  The HOST centroids given at create are history from here on.
 * ADMPC_EINVAL, in this order: a null ensemble; a null array. */
int admpc_quad_clusters_install(AdmpcQuadEnsemble* e, const double* gmm, const int32_t* info, int32_t* perm, int32_t* installed, void* stream);

/* Device [K][n_feat] <-> the ensemble's device centroids, on the stream.  set is a one-wave kernel: installed [1] int32 = 1 and the
 * centroids written if every value is finite, else 0 and the centroids stay.  get is a copy.
 * ADMPC_EINVAL, in this order: a null ensemble; a null array. */
int admpc_quad_ensemble_centroids_set(AdmpcQuadEnsemble* e, const double* centroids, int32_t* installed, void* stream);
int admpc_quad_ensemble_centroids_get(const AdmpcQuadEnsemble* e, double* centroids, void* stream);

/* `steps` launches of admpc_quad_ensemble_bin_kernel, one per logged step log[t] ([steps][B][14]), in order: onto zeroed bins
 * [K][3][32][5] and dropped [K][4] they leave, bit for bit, what an observed flight of those records under the PRESENT centroids would
 * have accumulated.
 * ADMPC_EINVAL, in this order: a null ensemble; an ensemble created without observe parameters; steps < 0 or B < 0; then (steps > 0 and
 * B > 0) a null array. */
int admpc_quad_clusters_rebin(const AdmpcQuadEnsemble* e, int steps, int B, const double* log, double* bins, int32_t* dropped, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_CLUSTERS_H */
