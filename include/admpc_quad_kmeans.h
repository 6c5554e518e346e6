/*
 * admpc_quad_kmeans.h -- the stage in front of the Gaussian-mixture EM of admpc_quad_clusters.h, on the device (libadmpc.so;
 * csrc/admpc_quad_kmeans.hip): scikit-learn's greedy k-means++ seeding and its Lloyd k-means over the logged sample records, whose
 * centres are the means the EM starts from, and the n_init rule that keeps the best of several fits.  With it nothing about the clusters
 * of a flight is given by hand: record -> prune -> k-means -> EM -> install -> re-bin is one chain of launches on one stream.  An addition
 * to admpc_quad_clusters.h, whose conventions hold here: device pointers owned by the caller, dense, fp64; `stream` a hipStream_t passed
 * as void*; 0 or a negative ADMPC_E* code returned, admpc_last_error() of admpc.h for the message; the caller's HIP device restored; no
 * host synchronisation and no allocation in any entry, each of which can be captured into a graph; every refusal in front of the first
 * device call, in the order it is listed; M == 0 is a no-op.
 *
 *   reference call site (data_driven_mpc/ros_gp_mpc/src/...)                                  replaced by
 *   ----------------------------------------------------------------------------------------  ------------------------------------
 *   model_fitting/gp_common.py:242    GaussianMixture(n_clusters).fit(x_pruned): with the      admpc_quad_kmeans_fit, then
 *                                     defaults of scikit-learn 1.7.2, init_params="kmeans":    admpc_quad_clusters_fit(init = centers)
 *     sklearn.cluster._kmeans._kmeans_plusplus      the greedy k-means++ seeding               the seeding rounds of admpc_quad_kmeans_fit
 *     sklearn.cluster.KMeans(n_clusters, n_init=1), _kmeans_single_lloyd                        its Lloyd iterations
 *     sklearn.mixture.GaussianMixture(n_init=n): the fit with the largest lower bound           admpc_quad_clusters_keep, admpc_quad_kmeans_keep
 *
 * NOT offered: the other init_params of scikit-learn; sample weights; Elkan's algorithm; choosing K.  AN EMPTY CLUSTER IS A FAILURE: where a
 * labelling pass leaves cluster k without a record, scikit-learn relocates the centre to a far point; here the fit ends with status
 * -(k + 1).  This is a deliberate difference.
 *
 * THE RECORDS are admpc_quad_learn.h's [14], packed by the EM's pack kernel (admpc_quad_clusters.h) as it is: a record counts if its
 * flag is 1.0 and its d = n_feat clustering features are finite; n_valid is their number; "log order" is the order of the record index.
 *
 * THE RANDOM NUMBERS.  Philox4x32-10 as admpc_quad_noise.h has it, key (seed low 32 bits, seed high 32 bits), counter (round c, draw,
 * call j, ADMPC_KMEANS_PHILOX_WORD).  The four output words o of a call give w0 = o0 | o1 << 32 and w1 = o2 | o3 << 32, and a word
 * u = ((double)(w >> 11) + 0.5) * 2^-53, in (0, 1).  Round 0 uses word 0 of call 0; trial t of round c >= 1 uses word t % 2 of call t / 2.
 *
 * THE SEEDING (greedy k-means++, _kmeans_plusplus with unit weights).  Round 0: centre 0 is the r-th counting record in log order,
 * r = min(floor(u n_valid), n_valid - 1), found through an exact integer prefix count of the flags (the count of every tile of 256
 * records, a one-wave scan, a walk inside one tile).  D2_i = ((x0 - c0)^2 + (x1 - c1)^2) + (x2 - c2)^2, the features past d at 0, every
 * operation rounded on its own, no contraction; the potential is the sum of D2 over the counting records.  Round c = 1 .. K - 1 draws
 * T = 2 + int(ln K) trials (2, 2, 3, .., 3, 4 for K = 1, 2, 3, .., 7, 8): with tau_t = u_t * potential the candidate is the first counting
 * record whose inclusive cumulative sum of D2, in log order, is >= tau_t, the last counting record if there is none (where rounding alone hides the crossing inside the tile the tile sums point
 * to, that tile's last counting record) -- by sums over
 * contiguous tiles of 256 records, a one-wave scan of the tile sums and a walk inside the one tile.  A candidate's potential is
 * sum_i min(D2_i, d2(x_i, x_cand)), through one row of partial sums per block and a one-wave finish; the smallest wins, ties to the lower
 * trial; its minimum is the new D2, its potential the new potential, its record index idx[c].
 *
 * LLOYD (_kmeans_single_lloyd).  Every iteration labels every counting record by quad_nearest (csrc/quad_route_dev.h: the routing's
 * arithmetic, ties to the lower index) and moves every centre to the mean of its records, the moments taken about the CURRENT centre:
 * c <- c + sum (x - c) / N.  shift = sum_k |c_new - c_old|^2.  Stop with converged = 2 if no label changed against the iteration before
 * (the first iteration changes all), else with converged = 1 if shift <= tol_abs = tol * mean_j var_j(X), the population variance per
 * feature over the counting records (one reduction at the start, the moments about record 0).  After a stop by tolerance or at max_iter
 * one more labelling pass makes the labels consistent with the final centres.  iterations is scikit-learn's n_iter_.
 *
 * THE RESULTS.  centers [K][d]; idx int64 [K] the record indices of the seeding; labels int32 [M], -1 for a record that does not count;
 * stats [4]: the inertia (the sum of squared distances to the record's centre), tol_abs, the last shift, the potential after seeding;
 * info int32 [4]: iterations, converged (0, 1, 2), status, n_valid.  status: 0; ADMPC_GMM_ENOVALID if no record counts;
 * ADMPC_KMEANS_EFEW if n_valid < K or the potential is 0 before K centres are placed (fewer than K distinct points); -(k + 1) for the
 * lowest cluster k that a labelling pass left empty (iterations then counts the iterations before that pass; labels are left as the passes
 * wrote them).  A failure stops the launches behind it, leaves stats at 0 and writes the ensemble's
 * PRESENT device centroids into centers, so that an EM chained behind it starts where it would have started without this stage.
 *
 * DETERMINISM.  No floating-point atomics; the one atomic counts changed labels, in integers.  The grid of every kernel over the records is
 * min(ceil(M / 256), ADMPC_GMM_BLOCKS_MAX) blocks of 256 threads, a function of M alone; every block writes one row of partial, and one
 * wave adds the rows in a fixed order.  4 K + 2 max_iter + 3 launches (pack, prep, seed0; per round pick -- not in round 0 --, the
 * candidates' potentials, the finish, the update of D2 -- not in the last round --; per iteration assign and move; the last pass and the
 * end), a function of K and max_iter alone: once converged or failed, the remaining launches read the flag and return at once.  Two runs
 * on the same input give the same bits.  The order inside the sums is not part of the contract: idx, labels, iterations and converged
 * are those of the rule above wherever no threshold lies within rounding of a cumulative sum, no two candidate potentials and no two
 * centre distances of a record within rounding of each other (tests/quad_kmeans_spec.py reports this margin per case).
 *
 * ACCURACY against the rule in 80-bit arithmetic, with u = 2^-53 and n_k the records of cluster k: a centre coordinate within
 * u max_j |c_j| + (n_k + 3) u max_i |x_i - c| (the centre is c + S / N in doubles), the inertia within (n + 4) u inertia, tol_abs within (n + 6) u tol (S2 / n + s^2) summed over the
 * features, S2 and s the second moment and the mean about record 0 (about zero if record 0 does not count).  That pivot is one record,
 * not the mean: for a log that lies far from it with a small spread, S2 / n - s^2 cancels and tol_abs loses the digits that |s| / sigma
 * has squared -- the bound says so, and tol_abs can then be far less accurate than the other results; it only places the stop by
 * tolerance.  Worst measured fractions of these bounds on one MI355X
 * (tests/test_quad_kmeans_gpu.py, M = 63 .. 65 793, K = 1 .. 8, d = 1 .. 3): centres 0.235, inertia 0.014, tol_abs 0.005.
 *
 * Measured on one MI355X at B = 4096, 60 logged steps (M = 245 760 records), K = 4, on d = 1 (the body-frame v_x) / d = 3 (the body-frame
 * velocity), captured graphs replayed, both routes alternating in one session, medians of three (scripts/quad_kmeans_time.py; DESIGN
 * section 7), microseconds: one Lloyd iteration (assign and move) 31.2 / 35.3; pack, prep, seed0, the 14 launches of the seeding rounds and the last pass
 * 212 / 211; what init="kmeans" adds to a fleet's fit_clusters() at scikit-learn's defaults (619 launches, of which 4 / 30 Lloyd
 * iterations ran and the rest return at once) 1270 / 2019, the whole call 7880 / 10 441.  The route it replaces -- the log to the host
 * 5606 / 1498, KMeans(n_init=1) from the same seeded points 23 951 / 89 707 (4 / 30 iterations too, its centres within 2.7e-15 of the
 * device's), the upload 272 / 258 -- 29 829 / 91 463: 23 / 45 times as long.  The kernel-trace split is UNMEASURED.  `make resources`
 * (VGPRs, LDS bytes per block; no kernel has scratch or spills): prep 34, 48; seed0 46, 512; cand 30, 32; finish 20, 512; update 23, 32;
 * pick 49, 0; assign<K, false> 34 / 66 / 76 / 86 / 96 / 110 / 124 / 138 for K = 1 .. 8, 56 .. 224; move 64, 512; end 20, 512; keep 8, 0.
 */
#ifndef ADMPC_QUAD_KMEANS_H
#define ADMPC_QUAD_KMEANS_H

#include <stdint.h>
#include "admpc_quad_clusters.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ADMPC_KMEANS_PHILOX_WORD 0x4B4D2B2Bu     /* the fourth counter word of every draw: "KM++" */
#define ADMPC_KMEANS_PARTIAL 33                 /* doubles per row of partial: count and first moment [3] of 8 clusters, and the inertia */
#define ADMPC_KMEANS_STATE 48                   /* doubles of state at the end of work */
#define ADMPC_KMEANS_EFEW (-101)
/* doubles of `work` for M records: the sum and the count of every tile, ADMPC_GMM_BLOCKS_MAX rows of partial, the state */
#define ADMPC_KMEANS_WORK(M) (2 * (((M) + 255) / 256) + ADMPC_GMM_BLOCKS_MAX * ADMPC_KMEANS_PARTIAL + ADMPC_KMEANS_STATE)

/* records [M][14] -> centers, idx, labels, stats, info (THE RESULTS above) under seed and draw, K, d and the features the ensemble's.
 * packed [M][4], dist [M], labels int32 [M] and work [ADMPC_KMEANS_WORK(M)] are the caller's; packed is left as the EM's pack leaves it.
 * ADMPC_EINVAL, in this order: a null ensemble; a clustering feature outside 7 .. 16 (the record holds no others); max_iter outside
 * 1 .. 1000; a tol that is negative or not finite; M < 0; then (M > 0) a null array. */
int admpc_quad_kmeans_fit(const AdmpcQuadEnsemble* e, uint64_t seed, uint32_t draw, int max_iter, double tol, int64_t M, const double* records,
                          double* packed, double* dist, int32_t* labels, double* work, double* centers, int64_t* idx, double* stats,
                          int32_t* info, void* stream);

/* One wave: scikit-learn's n_init rule over two states of admpc_quad_clusters_fit.  The try replaces the best if its status is 0 and its
 * lower bound is finite, and either the best holds nothing yet or the try's bound is strictly larger.  kept [1] int32 is the draw whose
 * fit the best holds, -1 while it holds none; draw == 0 starts a series: the best is taken to hold nothing, and a try that is not good
 * is copied all the same, so that the best carries its status.
 * ADMPC_EINVAL, in this order: a null ensemble; a negative draw; a null array. */
int admpc_quad_clusters_keep(const AdmpcQuadEnsemble* e, int draw, const double* gmm_try, const int32_t* info_try, double* gmm_best,
                             int32_t* info_best, int32_t* kept, void* stream);

/* Behind admpc_quad_clusters_keep of the same draw: the k-means results of the try (centers [K][d], idx [K], labels [M], stats [4], info [4])
 * copied into those of the best if that call kept the try's mixture (kept[0] == draw) or started a series (draw == 0), so that they
 * describe the fit the best mixture came from.  The grid is the fit's.
 * ADMPC_EINVAL, in this order: a null ensemble; a negative draw; M < 0; then (M > 0) a null array. */
int admpc_quad_kmeans_keep(const AdmpcQuadEnsemble* e, int draw, int64_t M, const int32_t* kept, const double* centers_try, const int64_t* idx_try,
                           const int32_t* labels_try, const double* stats_try, const int32_t* info_try, double* centers, int64_t* idx,
                           int32_t* labels, double* stats, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADMPC_QUAD_KMEANS_H */
